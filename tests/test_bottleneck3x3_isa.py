"""CPU: the fused 32-channel Bottleneck kernel (csrc/conv3x3.hip, bottleneck3x3_c32_kernel) in the gfx950 code object
(hipcc -S, no GPU): no scratch, the VGPRs of a 512-thread workgroup (two waves per SIMD: 256), the LDS size DESIGN.md
states, and the occupancy that follows: one workgroup per CU. Only the kernel descriptors' metadata is read."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "yolo-sod_amd" / "csrc"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)

THREADS = 512
LDS_BYTES = 157696        # 2 x 46,080 (input planes) + 2 x 32,640 (intermediate planes) + 256 (biases)
CU_LDS = 160 * 1024
SIMD_VGPRS = 512          # unified VGPR / AGPR file per SIMD lane


def _descriptors(tmp_path):
    out = tmp_path / "conv3x3.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", f"-I{CSRC}",
                    "-o", str(out), str(CSRC / "conv3x3.hip")], check=True, capture_output=True, timeout=600)
    text = out.read_text()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)", text):
        desc = text[m.start():text.find(".end_amdhsa_kernel", m.start())]
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\d+)\s*$", desc, re.M)}
    return res


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_fused_bottleneck_kernel_resources(tmp_path):
    ds = {n: d for n, d in _descriptors(tmp_path).items() if "bottleneck3x3_c32_kernel" in n}
    assert len(ds) == 2, sorted(ds)  # with and without the shortcut
    waves_per_simd = THREADS // 64 // 4
    for name, d in sorted(ds.items()):
        print(f"{name}: {d['next_free_vgpr']} VGPRs, LDS {d['group_segment_fixed_size']}, "
              f"scratch {d['private_segment_fixed_size']}")
        assert d["private_segment_fixed_size"] == 0, name
        assert d["next_free_vgpr"] <= SIMD_VGPRS // waves_per_simd, name
        assert d["group_segment_fixed_size"] == LDS_BYTES <= CU_LDS, name
        assert CU_LDS // d["group_segment_fixed_size"] == 1, name  # one workgroup per CU, two waves per SIMD
    assert f"{LDS_BYTES:,}" in (ROOT / "DESIGN.md").read_text()
