"""CPU: resources of the statistics forms of the fp16-split 1x1 conv kernel (conv1x1_x2s_kernel<CPW, STATS>,
csrc/conv1x1x2.hip) from the kernel descriptors' metadata of a hipcc -S build for gfx950, no GPU: no scratch, no
spills, at most 256 VGPRs (two 256-thread workgroups per CU) and one pair of staged planes of LDS, which is what the
plain forms they stand beside have. Only the metadata is read, not the instruction text."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "yolo-sod_amd" / "csrc"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)
PLANES = 2 * 64 * (128 + 8) * 2  # bytes of one pair of planes
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    out = tmp_path_factory.mktemp("c1sisa") / "conv1x1x2.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "--cuda-device-only", "-S", f"-I{CSRC}",
                    f"-I{ROOT / 'include'}", "-o", str(out), str(CSRC / "conv1x1x2.hip")], check=True,
                   capture_output=True, timeout=600)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    ks = {}
    for blk in re.split(r"\n  - (?=\.agpr_count:)", meta)[1:]:
        f = {k: v for k, v in re.findall(r"^\s*\.(\w+):\s+(\S+)$", blk, re.M)}
        ks[f.get("name", "")] = f
    return ks


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_every_statistics_instance_fits(descriptors):
    got = set()
    for name, f in descriptors.items():
        m = re.search(r"conv1x1_x2s_kernelILi(\d)ELi(\d)EE", name)
        if not m:
            continue
        cpw, stats = (int(v) for v in m.groups())
        got.add((cpw, stats))
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, name
        assert int(f["vgpr_count"]) <= 256 and int(f["agpr_count"]) == 0, (name, f["vgpr_count"], f["agpr_count"])
        assert int(f["group_segment_fixed_size"]) == PLANES and 2 * PLANES <= LDS_PER_CU, name
        assert int(f["max_flat_workgroup_size"]) == 256, name
    # <CPW, STATS>: workgroups of 128 and of 256 output channels, each with the sum and with the sum and the max
    assert got == {(2, 1), (2, 2), (4, 1), (4, 2)}, got


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_statistics_forms_cost_no_more_registers_than_two_workgroups_allow(descriptors):
    """The plain instance of the same shape beside each statistics instance: the statistics add a handful of
    registers at most and stay in the same occupancy class (<= 256 VGPRs: two workgroups of four waves per CU)."""
    plain = {int(re.search(r"ELi64ELi(\d)ELb0EE", n).group(1)): int(f["vgpr_count"]) for n, f in descriptors.items()
             if re.search(r"conv1x1_x2_kernelILb0ELi64ELi\dELb0EE", n)}
    for name, f in descriptors.items():
        m = re.search(r"conv1x1_x2s_kernelILi(\d)ELi(\d)EE", name)
        if m:
            assert int(f["vgpr_count"]) <= min(256, plain[int(m.group(1))] + 16), (name, f["vgpr_count"], plain)
