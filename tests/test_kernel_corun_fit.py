"""What the co-run of the pack kernel rests on, as the compiler reports it (no GPU needed): a pack workgroup -- four waves, one
per SIMD -- must fit on a CU beside THREE main-tier workgroups of the wave kernel, in registers and in LDS, and neither kernel
may use scratch.  A vector-register allocation comes in steps of 8 per lane, a SIMD has 512 per lane, a CU 160 KiB of LDS.
These are conditions from that arithmetic, not measurements: the day one of the two kernels outgrows them, a large batch's
pack kernel on the ingest stream goes back to taking turns with the wave kernel ("Streams")."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import CSRC

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
PACK = "_Z14vg_pack_kernelPKhS0_PKmmPmS3_PjPKjS6_j"
MAIN = "_ZN2vg14vg_wave_kernelILb0ELi14ELi6ELi4ELb0EEE"          # vg_wave_kernel<false, 14, 6, 4, false>: the headline instantiation


def _resources(tmp_path):
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-pass-failed",
                          "-DVG_LIB_BUILD_ID=\"test\"", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "dev.o"), os.path.join(CSRC, "vargeno_hip.hip")],
                         capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, out.stderr[-4000:]
    res, name = {}, None
    for ln in out.stderr.splitlines():
        m = re.search(r"remark: *([^:]+?): *(\S+)", ln)
        if not m:
            continue
        k, v = m.group(1).split("[")[0].strip(), m.group(2)
        if k == "Function Name":
            name = v
            res[name] = {}
        elif name is not None:
            res[name][k] = v
    return res


@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_a_pack_workgroup_fits_beside_three_main_tier_workgroups(tmp_path):
    res = _resources(tmp_path)
    pack = res[PACK]
    mains = [v for k, v in res.items() if k.startswith(MAIN)]
    assert len(mains) == 1, [k for k in res if "vg_wave_kernel" in k]
    main = mains[0]
    up8 = lambda v: (int(v) + 7) // 8 * 8
    print("pack kernel:", pack, "\nmain tier:", main)
    assert int(pack["ScratchSize"]) == 0 and int(main["ScratchSize"]) == 0
    # a workgroup of either kernel has four waves, one per SIMD: per SIMD, three main-tier waves and one pack wave
    assert 3 * up8(main["VGPRs"]) + up8(pack["VGPRs"]) <= 512, (main["VGPRs"], pack["VGPRs"])
    lds = lambda r: int(r["LDS Size"])
    assert 3 * lds(main) + lds(pack) <= 160 * 1024, (lds(main), lds(pack))
