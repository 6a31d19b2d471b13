"""CPU: the persistent 3x3 conv kernel's halo staging in the gfx950 code object (hipcc -S, no GPU). The staging loads
aligned groups of four pixels with one 16-byte buffer load per channel (csrc/conv3x3.hip, YS_C3_WIDE_STAGE): no
instance may keep a 4-byte buffer load (the kernel's only buffer loads are the halo and the weight fragments, 16 bytes
each), spill, pass 256 VGPRs or change its LDS size (two workgroups per CU: at most 80 KB each)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "yolo-sod_amd" / "csrc"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)

# group segment bytes per tile geometry (template argument G) with the one-load-per-pixel staging: two fp16 planes of
# HH x RS pixels x 48 halves + 512 bias floats
LDS_BYTES = {0: 67328, 1: 77312, 2: 75776}


def _instances(src, pattern, tmp_path):
    out = tmp_path / (src + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "--cuda-device-only", "-S", f"-I{CSRC}", "-o", str(out),
                    str(CSRC / src)], check=True, capture_output=True, timeout=300)
    text = out.read_text()
    res = {}
    for m in re.finditer(r"^(_Z[^:\s]+):", text, re.M):
        name = m.group(1)
        if pattern not in name:
            continue
        body = text[m.end():text.find("s_endpgm", m.end())]
        d = text.find(".amdhsa_kernel " + name)
        desc = text[d:text.find(".end_amdhsa_kernel", d)]
        res[name] = (body, {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\d+)\s*$", desc, re.M)})
    return res


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_conv3x3_p_kernel_stages_with_16_byte_loads(tmp_path):
    ks = _instances("conv3x3.hip", "conv3x3_p_kernel", tmp_path)
    assert len(ks) == 12, sorted(ks)  # 3 geometries x 2 group widths x residual or not
    for name, (body, desc) in sorted(ks.items()):
        geo = int(re.search(r"conv3x3_p_kernelILi(\d)E", name).group(1))
        n4 = len(re.findall(r"\bbuffer_load_dword\s", body))
        n16 = len(re.findall(r"\bbuffer_load_dwordx4\s", body))
        print(f"{name}: {desc['next_free_vgpr']} VGPRs, LDS {desc['group_segment_fixed_size']}, "
              f"{n16} 16-byte / {n4} 4-byte buffer loads")
        assert desc["private_segment_fixed_size"] == 0, name
        assert desc["next_free_vgpr"] <= 256, name
        assert desc["group_segment_fixed_size"] <= 81920, name
        assert desc["group_segment_fixed_size"] == LDS_BYTES[geo], name
        assert n4 == 0, f"{name}: {n4} 4-byte buffer loads left"
        assert n16 > 0, name
