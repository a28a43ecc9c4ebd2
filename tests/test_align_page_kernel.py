"""No GPU: what the compiler reports for every instantiation of `ctc_align_page_kernel` (csrc/ctc_align_page.hip.h, DESIGN.md section
7n).  The kernel's frame loop is one serial chain per page, so a spill inside it is paid 12 000 times per page: the scratch of every
offered form is held at 0 here.  (A form of 16 registers per lane, for texts of 4096 .. 8191 labels, did not meet this and is not
offered.)"""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = (1, 2, 4, 8)
ARGS = ('const float *, int, int, const int32_t *, const int32_t *, const int32_t *, const int32_t *, const int32_t *, const uint32_t *, unsigned *, int, '
        'int32_t *, int32_t *, int32_t *, float *, float *, int32_t *, float *')


def test_every_form_compiles_without_scratch(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc)
    unit = tmp_path / 'forms.hip'
    unit.write_text('#include "ctc_align_page.hip.h"\n'
                    + ''.join(f'template __global__ void ctc_align_page_kernel<{sj}>({ARGS});\n' for sj in FORMS))
    from conformer_ocr_amd.build import ARCH
    r = subprocess.run([hipcc, f'--offload-arch={ARCH}', '-O3', '-std=c++17', '-fno-gpu-rdc', '-mllvm', '-amdgpu-mfma-vgpr-form', '--cuda-device-only',
                        '-I', os.path.join(ROOT, 'conformer_ocr_amd', 'csrc'), '-I', os.path.join(ROOT, 'include'),
                        '-Rpass-analysis=kernel-resource-usage', '-c', str(unit), '-o', str(tmp_path / 'forms.o')],
                       stderr=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows, cur = {}, None
    for l in r.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', l)
        if m:
            cur = rows.setdefault(m.group(1), {})
        for key, pat in (('vgprs', 'VGPRs'), ('scratch', r'ScratchSize \[bytes/lane\]'), ('spilled', 'VGPRs Spill')):
            m = re.search(r'remark: .*?\b' + pat + r': (\d+)', l)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    forms = {int(re.search(r'ctc_align_page_kernelILi(\d+)E', n).group(1)): v for n, v in rows.items() if 'ctc_align_page_kernel' in n}
    print(forms)
    assert sorted(forms) == list(FORMS)
    for sj, v in forms.items():
        assert v['scratch'] == 0 and v['spilled'] == 0, (sj, v)
        assert v['vgprs'] <= 128, (sj, v)                                 # 16 waves of one workgroup on a CU
    # the host side offers exactly these forms: the largest text the entry takes has 2 * 4095 + 1 states = 16 waves x 8 registers x 64 lanes
    with open(os.path.join(ROOT, 'conformer_ocr_amd', 'csrc', 'ctc_align_page.hip.h')) as fp:
        src = fp.read()
    assert re.search(r'#define COCR_PAGE_MAX_LABELS (\d+)', src).group(1) == '4095' and 'while (sj < 8 &&' in src
