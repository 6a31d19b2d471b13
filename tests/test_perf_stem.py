"""perf accounting of the stem kernel's launch key ("stem", x shape, (cout, "sum")): it is the producer of SE L1's
statistics, its plain pass is priced at the HBM roof of its own bytes, and it is listed with the backbone ops, outside
the path roofline (CPU only; the numbers are synthetic)."""
import pytest

import yolosod_import  # noqa: F401
from yolosod_amd import perf

STEM = ("stem", (32, 3, 640, 640), (32, "sum"))
STEM_BYTES = (32 * 3 * 640 * 640 + 32 * 32 * 320 * 320) * 4
ROOF_MS = STEM_BYTES / 8e12 * 1e3


def test_stem_is_the_producer_of_the_se_after_it():
    gate, gshape, plain, nbytes = perf.producer_of(STEM)
    assert (gate, gshape, nbytes) == ("se", (32, 32, 320, 320), STEM_BYTES)
    assert plain[0] == "stem" and plain != STEM
    assert perf.producer_of(("stem", (32, 3, 640, 640), (32, None))) is None
    billed = perf.producer_billing(perf.aggregate([(STEM, 0.2), (STEM, 0.22)]))
    ext, src = billed[("se", (32, 32, 320, 320))]
    assert ext == pytest.approx(0.21 - ROOF_MS) and "HBM roof" in src


def test_stem_is_a_backbone_op_billed_to_the_fused_se_conv():
    gate = ("se_gate", (32, 32, 320, 320), 8)
    fused = ("se_conv", (32, 32, 320, 320), (64, 8))
    assert "stem" not in perf.PATH_OPS and perf.PathSelect()(STEM)
    ops, backbone, path = perf.summarize([(STEM, 0.2), (gate, 0.005), (fused, 0.14)], steps=1)
    assert [(b["op"], b["shape"], b["launches"]) for b in backbone] == [("stem", [32, 3, 640, 640], 1)]
    assert [o["op"] for o in ops] == ["se_conv"]
    assert ops[0]["avg_ms"] == pytest.approx(0.145 + 0.2 - ROOF_MS, abs=1e-4)
    assert ops[0]["producer_extra_ms"] == pytest.approx(0.2 - ROOF_MS, abs=1e-4)
