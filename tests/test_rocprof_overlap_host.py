"""tools/summarize_rocprof.py overlap: forwards per hardware queue and forwards executing at once, on a hand-made kernel trace."""
import csv
import io
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = '_Z17frontend96_kernelIfEvPKT_'
CHAIN = 'void rowchain_kernel<256, 4, 31, 0, 1, 1, 3, false, 8, 8>(ChainArgs)'


def test_overlap_counts_forwards_per_queue_and_at_once(tmp_path):
    """Queue 1 carries two streams: its forwards run back to back, 100 us each (frontend 40 us + chain 60 us).  Queue 2 carries one stream:
    one forward per two of queue 1's, at the same time as every second one.  Steady half: 8 forwards on queue 1 (800 us, no gaps), 4 on
    queue 2 -> 1200 us of forwards in 800 us of wall = 1.5 at once; the chain launch has 9600 / 64 = 150 workgroups of 512 threads."""
    rows, did = [], 0

    def forward(q, t):
        nonlocal did
        for name, s, e, grid in ((FRONT, t, t + 40_000, 256 * 300), (CHAIN, t + 40_000, t + 100_000, 150 * 512)):
            did += 1
            rows.append({'Kind': 'KERNEL_DISPATCH', 'Agent_Id': 1, 'Queue_Id': q, 'Kernel_Name': name, 'Dispatch_Id': did,
                         'Start_Timestamp': 1_000_000 + s, 'End_Timestamp': 1_000_000 + e, 'Workgroup_Size_X': 512 if name == CHAIN else 256,
                         'Grid_Size_X': grid})
    for i in range(16):
        forward(1, 100_000 * i)
        if i % 2 == 0:
            forward(2, 100_000 * i)
    rows.sort(key=lambda r: r['Start_Timestamp'])
    d = tmp_path / 'out' / 'host'
    d.mkdir(parents=True)
    with open(d / '123_kernel_trace.csv', 'w', newline='') as fp:
        w = csv.DictWriter(fp, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'summarize_rocprof.py'), 'overlap', str(tmp_path / 'out')],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = {(x['what'], x['key']): x for x in csv.DictReader(io.StringIO(r.stdout))}
    assert got[('queue forwards', '1')]['count'] == '8' and float(got[('queue forwards', '1')]['value']) == 2.0
    assert got[('queue forwards', '2')]['count'] == '4' and float(got[('queue forwards', '2')]['value']) == 1.0
    assert float(got[('queue forward span', '1')]['value']) == 100.0
    assert float(got[('queue busy', '1')]['value']) == 1.0 and float(got[('queue busy', '2')]['value']) == 0.5
    assert got[('queues with forwards', '')]['value'] == '2'
    assert float(got[('forwards executing at once', '')]['value']) == 1.5
    assert float(got[('kernels executing at once', '')]['value']) == 1.5
    assert float(got[('forward rate', '')]['value']) == 15000.0
    chain = got[('chain launch', 'void rowchain_kernel<256, 4, 31, 0, 1, 1, 3, false, 8, 8>')]
    assert chain['count'] == '12' and float(chain['value']) == 60.0 and chain['unit'] == 'us mean, 150 workgroups'
