"""CPU: what the compiler made of the evaluator's matching kernel (hipcc -S for gfx950, no GPU). A workgroup belongs
to one image, so the image's count and its two label offsets are read with scalar loads (no vector load made uniform
afterwards, no waterfall loop); the kernel uses no scratch (the sixteen thresholds are indexed with constants after
unrolling, never through a private array), and the IoU is an IEEE division."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "yolo-sod_amd" / "csrc"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_eval_match_kernel_offsets_are_scalar_loads_and_nothing_spills(tmp_path):
    out = tmp_path / "eval_match.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--cuda-device-only", "-S",
                    f"-I{CSRC}", "-o", str(out), str(CSRC / "eval_match.hip")], check=True, capture_output=True,
                   timeout=300)
    text = out.read_text()
    bodies = {}
    for m in re.finditer(r"^(_Z[^:\s]+):", text, re.M):
        bodies[m.group(1)] = text[m.end():text.find("s_endpgm", m.end())]
    ks = {k: v for k, v in bodies.items() if "eval_match_kernel" in k}
    assert len(ks) == 1, list(bodies)
    body = next(iter(ks.values()))
    rfl, loops = body.count("v_readfirstlane"), body.count("s_cbranch_execnz")
    assert rfl <= 16 and loops <= 16, f"{rfl} readfirstlane, {loops} exec-mask loops (waterfall loads?)"
    # scalar loads: (destination, base pair, offset). The first one reads the kernel arguments; the loads from any other
    # base are counts[b] (one dword) and label_off[b], label_off[b + 1] (one two-dword load)
    loads = re.findall(r"s_load_dword(x\d+)?\s+s\[?[\d:]+\]?,\s*(s\[\d+:\d+\]),", body)
    assert loads, "no scalar loads at all"
    kernarg = loads[0][1]
    other = [width for width, base in loads if base != kernarg]
    assert "" in other, f"counts[b] is not read with a scalar load: {loads}"
    assert "x2" in other, f"label_off[b], label_off[b + 1] are not read with one scalar load: {loads}"
    assert "v_div_scale_f32" in body, "the IoU is an IEEE division"
    assert "ds_read_b128" in body, "the staged label boxes are read 16 bytes at a time"
    scratch = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert scratch and all(int(v) == 0 for v in scratch), scratch
    lds = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text)
    assert lds and all(int(v) <= 16384 for v in lds), lds
