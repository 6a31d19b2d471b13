"""CPU: what the compiler made of the fused branch-merge kernel (hipcc -S for gfx950, no GPU). A workgroup belongs to
one destination slot, so the slot's descriptor row is read with scalar loads and no load sits in a waterfall loop
(tests/test_isa_guard.py); the kernel uses no scratch, and both divisions of a box term are IEEE divisions."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "yolo-sod_amd" / "csrc"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_tile_merge_tta_kernel_descriptor_loads_are_uniform_and_nothing_spills(tmp_path):
    out = tmp_path / "tile_merge_tta.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--cuda-device-only", "-S",
                    f"-I{CSRC}", "-o", str(out), str(CSRC / "tile_merge_tta.hip")], check=True, capture_output=True,
                   timeout=300)
    text = out.read_text()
    bodies = {}
    for m in re.finditer(r"^(_Z[^:\s]+):", text, re.M):
        bodies[m.group(1)] = text[m.end():text.find("s_endpgm", m.end())]
    ks = {k: v for k, v in bodies.items() if "tile_merge_tta_kernel" in k}
    assert len(ks) == 1, list(bodies)  # the element-wise form only
    for name, body in ks.items():
        rfl, loops = body.count("v_readfirstlane"), body.count("s_cbranch_execnz")
        assert rfl <= 16 and loops <= 16, f"{name}: {rfl} readfirstlane, {loops} exec-mask loops (waterfall loads?)"
        # the kernel arguments and the 11 descriptor dwords: at least one wide scalar load beyond the argument loads
        assert len(re.findall(r"s_load_dwordx(?:8|16)", body)) >= 2, f"{name}: descriptor not read with scalar loads"
        # four box terms through two divisions each (/ scale, then / gain), two v_div_scale_f32 per division: none
        # folded into one, none replaced by a multiplication with a reciprocal
        assert body.count("v_div_scale_f32") >= 16, f"{name}: the ways back are IEEE divisions"
        assert body.count("v_div_fixup_f32") >= 8, name
    scratch = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert scratch and all(int(v) == 0 for v in scratch), scratch
