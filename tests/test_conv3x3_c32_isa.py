"""CPU: the Cin 32 -> Cout 32 forms of the persistent 3x3 conv kernel (csrc/conv3x3.hip, conv3x3_c32_kernel: resident
weights F 1, both channel blocks per wave F 2) in the gfx950 code object (hipcc -S, no GPU): two workgroups per CU
need every instance without scratch, within 256 VGPRs and with the LDS size its geometry has in conv3x3_p_kernel.
Only the kernel descriptors' metadata is read."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "yolo-sod_amd" / "csrc"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


def _descriptors(tmp_path):
    out = tmp_path / "conv3x3.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "--cuda-device-only", "-S", f"-I{CSRC}", "-o", str(out),
                    str(CSRC / "conv3x3.hip")], check=True, capture_output=True, timeout=600)
    text = out.read_text()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)", text):
        desc = text[m.start():text.find(".end_amdhsa_kernel", m.start())]
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\d+)\s*$", desc, re.M)}
    return res


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_c32_instances_keep_two_workgroups_per_cu(tmp_path):
    ds = _descriptors(tmp_path)
    lds = {}  # geometry -> the parent form's LDS bytes (every conv3x3_p_kernel instance of a geometry has the same)
    for name, d in ds.items():
        m = re.search(r"conv3x3_p_kernelILi(\d)E", name)
        if m:
            lds.setdefault(int(m.group(1)), set()).add(d["group_segment_fixed_size"])
    assert sorted(lds) == [0, 1, 2] and all(len(v) == 1 for v in lds.values()), lds
    new = {n: d for n, d in ds.items() if "conv3x3_c32_kernel" in n}
    assert len(new) == 12, sorted(new)  # 3 geometries x residual or not x F 1 / F 2
    for name, d in sorted(new.items()):
        geo = int(re.search(r"conv3x3_c32_kernelILi(\d)E", name).group(1))
        print(f"{name}: {d['next_free_vgpr']} VGPRs, LDS {d['group_segment_fixed_size']}, "
              f"scratch {d['private_segment_fixed_size']}")
        assert d["private_segment_fixed_size"] == 0, name
        assert d["next_free_vgpr"] <= 256, name
        assert {d["group_segment_fixed_size"]} == lds[geo], name
