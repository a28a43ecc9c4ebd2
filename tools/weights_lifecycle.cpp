// Host-side check of csrc/weights.hip.h: the lifecycle of a set of weights (Weights: who reads it, who releases it) and the
// bookkeeping of the hipGraph cache (GraphCache), driven on the CPU with the two HIP calls of the header stubbed by malloc / free.
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/weights_lifecycle.cpp -o /tmp/weights_lifecycle && /tmp/weights_lifecycle
//
// Every step asserts that `users` is exact; the sanitizers see a read of released memory, a double free or a leak.
#include <cassert>
#include <cstdio>
#include <cstdlib>

typedef void *hipStream_t;
typedef void *hipGraphExec_t;
typedef unsigned short bf16_t;
#define COCR_POS_MAXLEN 5000
static int g_live = 0;       // device allocations and instantiated graphs alive
static void *dev_alloc(size_t n) { ++g_live; return malloc(n); }
static void dev_free(void *p) { --g_live; free(p); }
#define COCR_DEVICE_FREE(p) dev_free(p)
#define COCR_GRAPH_EXEC_DESTROY(e) dev_free(e)
#include "../conformer_ocr_amd/csrc/weights.hip.h"

// as much of a model as the lifecycle needs; create / finalize / share / destroy do what cocr_api.hip does with the set (forward: forward.hip's sync_weights)
struct cocr_model {
    WeightsRef w;
    unsigned long long seen_gen = 0;
};
static cocr_model *create() { cocr_model *m = new cocr_model(); weights_own(m->w, m, 0); return m; }
static void finalize(cocr_model *m, int dtype) {
    weights_own(m->w, m, 0);
    m->w->dtype = dtype;
    m->w->plan.total = dtype == 0 ? 64 : 128;
    m->w->blob = (unsigned char *)dev_alloc(m->w->plan.total);
}
static void forward(cocr_model *m) {      // (sync_weights: derived copies rebuilt where stale, then the blob is read)
    Weights &w = *m->w;
    assert(w.blob);
    if (w.stale()) {
        if (!w.packed) w.packed = (unsigned char *)dev_alloc(w.plan.total);
        if (!w.ptab) w.ptab = (unsigned char *)dev_alloc(16);
        if (!w.fpack) w.fpack = (bf16_t *)dev_alloc(16);
        w.packed_stale = w.ptab_stale = false;
        ++w.gen;
    }
    w.blob[w.plan.total - 1] = w.packed[w.plan.total - 1] = 1;
    m->seen_gen = w.gen;
}
static void share(cocr_model *m, cocr_model *owner) { assert(owner->w->blob && owner->w->owned_by(owner)); weights_join(m->w, m, owner->w); }
static void destroy(cocr_model *m) { weights_leave(m->w, m); delete m; }
static bool users_are(const cocr_model *m, std::initializer_list<cocr_model *> want) {
    return m->w->users == std::vector<cocr_model *>(want);
}

static void lifecycle() {
    cocr_model *o = create(), *a = create(), *b = create();
    assert(users_are(o, {o}) && !o->w->blob && o->w->owned_by(o));
    finalize(o, 0);
    assert(users_are(o, {o}) && o->w->blob);
    // share
    share(a, o); share(b, o);
    assert(a->w == o->w && b->w == o->w && users_are(o, {o, a, b}) && !a->w->owned_by(a));
    forward(a); forward(o); forward(b);
    assert(o->w->gen == a->seen_gen && a->seen_gen == b->seen_gen);
    // the owner finalizes again, also in the other compute dtype: the same object, new buffers, a new generation; the sharers follow
    const Weights *set = o->w.get();
    const unsigned long long gen = set->gen;
    finalize(o, 1);
    assert(o->w.get() == set && users_are(o, {o, a, b}) && set->gen > gen && set->stale() && !set->packed && a->w->dtype == 1 && a->w->blob == o->w->blob);
    forward(b); forward(a);
    // leave: a sharer finalized on weights of its own, a sharer destroyed
    finalize(a, 0);
    assert(users_are(o, {o, b}) && users_are(a, {a}) && a->w->owned_by(a) && a->w != o->w);
    forward(a); forward(o);
    destroy(b);
    assert(users_are(o, {o}));
    // sharer destroyed first, then the owner
    b = create(); share(b, o);
    assert(users_are(o, {o, b}));
    destroy(b);
    assert(users_are(o, {o}));
    // owner destroyed first: the set outlives it without device buffers and without users; the models that point at it are not
    // finalized, and get weights of their own (or another owner) afterwards
    b = create(); share(b, o);
    cocr_model *c = create(); share(c, o);
    WeightsRef orphaned = o->w;
    destroy(o);
    assert(b->w == orphaned && c->w == orphaned && !b->w->blob && !b->w->packed && b->w->users.empty() && !b->w->owned_by(b));
    finalize(b, 0);
    assert(users_are(b, {b}) && b->w != orphaned && orphaned->users.empty() && c->w == orphaned);
    forward(b);
    share(c, a);
    assert(users_are(a, {a, c}) && orphaned.use_count() == 1);
    forward(c);
    // an owner with sharers joins another set: its own set dies as if it had been destroyed
    cocr_model *d = create(); share(d, b);
    share(b, a);
    assert(users_are(a, {a, c, b}) && !d->w->blob && d->w->users.empty());
    destroy(d); destroy(a);
    assert(!c->w->blob && !b->w->blob && c->w->users.empty());
    destroy(c); destroy(b);
    orphaned.reset();
    assert(g_live == 0);
}

static hipGraphExec_t new_exec() { return dev_alloc(8); }
static void graph_cache() {
    typedef GraphCache G;
    char lines[64], logits[64];
    auto call = [&](int i, int N = 2, int rows = 96) { return G::Call{lines + i, (float *)logits + i, N, 300, 0, rows}; };
    hipGraphExec_t e = nullptr;
    {   // a caller that reuses its buffers: plain, captured on the second call once the shape is ready, then replayed
        G g;
        assert(g.next(call(0), false, &e) == G::PLAIN);
        assert(g.next(call(0), true, &e) == G::CAPTURE);
        hipGraphExec_t own = new_exec();
        g.add(call(0), own);
        assert(g.next(call(0), true, &e) == G::REPLAY && e == own);
        // other buffers, same shape: the staged sequence is captured on the second such call, then replayed
        assert(g.next(call(1), true, &e) == G::STAGED_CAPTURE);      // (the shape was seen with call(0))
        hipGraphExec_t st = new_exec();
        g.add(G::staged(call(1)), st);
        assert(g.next(call(2), true, &e) == G::STAGED_REPLAY && e == st);
        assert(g.next(call(0), true, &e) == G::REPLAY && e == own);
        // a new shape: plain first, even with the shape ready; not ready: plain again
        assert(g.next(call(3, 5), true, &e) == G::PLAIN);
        assert(g.next(call(4, 5), false, &e) == G::PLAIN);
        assert(g.next(call(5, 5), true, &e) == G::STAGED_CAPTURE);
        // another grid for a captured shape (a model joined or left the group): everything goes
        assert(g.next(call(0, 2, 64), true, &e) == G::PLAIN && g.graphs.empty() && g.seen.size() == 2);
    }
    {   // capacity: 16 sequences, the oldest evicted first; the seen calls lose their oldest from 32 on
        G g;
        std::vector<hipGraphExec_t> execs;
        for (int i = 0; i < 20; ++i) { execs.push_back(new_exec()); g.add(call(i), execs.back()); }
        assert(g.graphs.size() == 16 && g.graphs.front().exec == execs[4] && g.graphs.back().exec == execs[19]);
        for (int i = 20; i < 60; ++i) g.next(call(i), false, &e);
        assert(!G::same(g.seen.front(), call(20)) && G::same(g.seen.back(), G::staged(call(59))));
    }                                                        // (the destructor destroys what is left)
    assert(g_live == 0);
}

int main() {
    lifecycle();
    graph_cache();
    printf("weights lifecycle and graph cache: ok\n");
    return 0;
}
