"""GPU: the model's routing of the Detect towers' fused tail (modules.HEAD_FUSE, Detect.head_fuse_level / tower_into,
the executor's side streams): forced on, off and automatic give the same prediction tensor bit for bit; RawMaps of a
fused level equals the unfused path's raw maps; off, bf16 and exact_fp32_matrix() give the launch sequence without the
fused kernel; the non-executor path (Detect._fused_forward) and predict_padded agree."""
import pytest
import torch

from yolosod_amd import _hip
from yolosod_amd.nn import modules as M
from yolosod_amd.nn import tasks as T

pytestmark = pytest.mark.gpu


class forced:
    """yolosod_debug_set_conv3x3_head_fuse: -1 automatic, 0 never, 1 every shape."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = _hip.load_library().yolosod_debug_set_conv3x3_head_fuse(self.mode)

    def __exit__(self, *exc):
        _hip.load_library().yolosod_debug_set_conv3x3_head_fuse(self.old)


def _keys(m, x):
    with _hip.op_timer() as t:
        out = m(x)
    # the once-per-parameter-version weight preparations are not part of a step's launch sequence
    return out, [k for k, _ in t.durations_ms() if not k[0].endswith("_prep")]


def _is_tail(k):
    return k[0] == "conv3x3" and isinstance(k[2], tuple) and len(k[2]) == 3 and k[2][1] == "head"


@pytest.fixture(scope="module")
def runs(cuda):
    """The fp32 model at batch 2 and 256^2 under each setting (one forward each, outputs kept, never modified)."""
    from yolosod_amd.nn.tasks import build_model
    m = build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=cuda)
    mb = build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=cuda, dtype=torch.bfloat16)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(7)).to(cuda)
    out = dict(model=m, x=x)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.inference_mode():
            with forced(0):
                out["off"] = _keys(m, x)
            with forced(1):
                out["on"] = _keys(m, x)
                with _hip.exact_fp32_matrix():
                    out["exact_on"] = _keys(m, x)
                out["bf16_on"] = _keys(mb, x.to(torch.bfloat16))
                old = M.HEAD_FUSE
                M.HEAD_FUSE = False
                try:
                    out["switch_off"] = _keys(m, x)
                finally:
                    M.HEAD_FUSE = old
                M.Detect.keep_raw = True
                try:
                    out["raw"] = m(x)
                finally:
                    M.Detect.keep_raw = False
                streams = T.STREAMS
                T.STREAMS = 0  # no executor side streams: Detect._fused_forward
                try:
                    out["plain_on"] = _keys(m, x)
                finally:
                    T.STREAMS = streams
            with forced(0):
                with _hip.exact_fp32_matrix():
                    out["exact_off"] = _keys(m, x)
                out["bf16_off"] = _keys(mb, x.to(torch.bfloat16))
            out["auto"] = _keys(m, x)
    finally:
        torch.backends.cudnn.deterministic = det
    return out


def test_forced_on_off_and_automatic_agree(runs):
    (y0, _), k0 = runs["off"]
    (y1, _), k1 = runs["on"]
    (ya, _), ka = runs["auto"]
    assert torch.equal(y1, y0), float((y1 - y0).abs().max())
    assert torch.equal(ya, y0)
    assert not any(_is_tail(k) for k in k0)
    # forced on: every level's two towers end in the fused launch; their plain tower convs drop from 4 to 2 a level
    tails = [k for k in k1 if _is_tail(k)]
    assert len(tails) == 8 and sorted(k[2][2] for k in tails) == [1] * 4 + [2] * 4
    plain = lambda ks: sum(1 for k in ks if k[0] == "conv3x3" and not _is_tail(k))  # noqa: E731
    assert plain(k0) - plain(k1) == 8
    assert not any(k[0] == "head" for k in k1)
    assert sum(1 for k in k0 if k[0] == "head") == 1
    # automatic at batch 2: no level has enough tiles for 64-channel groups, the launches are the unfused ones
    assert ka == k0


def test_off_bf16_and_exact_take_the_unfused_launches(runs):
    assert runs["switch_off"][1] == runs["off"][1]
    assert torch.equal(runs["switch_off"][0][0], runs["off"][0][0])
    assert runs["exact_on"][1] == runs["exact_off"][1] and not any(_is_tail(k) for k in runs["exact_on"][1])
    assert runs["bf16_on"][1] == runs["bf16_off"][1] and not any(_is_tail(k) for k in runs["bf16_on"][1])
    assert torch.equal(runs["exact_on"][0][0], runs["exact_off"][0][0])
    assert torch.equal(runs["bf16_on"][0][0], runs["bf16_off"][0][0])


def test_non_executor_path(runs):
    (y, raw), keys = runs["plain_on"]
    assert torch.equal(y, runs["off"][0][0])
    assert sum(1 for k in keys if _is_tail(k)) == 8
    assert isinstance(raw, M.RawMaps)


def test_raw_maps_of_fused_levels(runs):
    """RawMaps keeps a fused level's input map and computes its features through tower_features on first access."""
    _, lazy = runs["on"][0]
    _, raw = runs["raw"]
    assert isinstance(lazy, M.RawMaps) and isinstance(raw, list) and len(lazy) == len(raw) == 4
    assert all(f is None for f in lazy._feats)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        maps = list(lazy)  # outside inference_mode: the inputs are inference tensors
    finally:
        torch.backends.cudnn.deterministic = det
    for a, b in zip(maps, raw):
        assert a.shape == b.shape and torch.equal(a, b)
    assert all(f is not None and f[0].shape[1] == 64 for f in lazy.features)


def test_mixed_levels(runs, cuda, monkeypatch):
    """Some levels fused, the others through the head kernel in one launch per run of levels, whose key carries the
    anchors it decodes."""
    m, x = runs["model"], runs["x"]
    pick = {0, 1}
    real = _hip.conv3x3_head_fused
    monkeypatch.setattr(_hip, "conv3x3_head_fused", lambda B, H, W: H in (64, 32))
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.inference_mode():
            (y, _), keys = _keys(m, x)
    finally:
        torch.backends.cudnn.deterministic = det
        monkeypatch.setattr(_hip, "conv3x3_head_fused", real)
    assert torch.equal(y, runs["off"][0][0])
    assert sum(1 for k in keys if _is_tail(k)) == 2 * len(pick)
    heads = [k for k in keys if k[0] == "head"]
    assert heads == [("head", (2, 16 * 16 + 8 * 8), (m.model[-1].nc, 64, 64))]


def test_predict_padded(runs, cuda):
    from yolosod_amd.engine.predictor import DetectionPredictor
    dp = DetectionPredictor(runs["model"], conf=0.001, imgsz=256)
    with forced(0):
        a = dp.predict_padded(runs["x"])
    with forced(1):
        b = dp.predict_padded(runs["x"])
    for u, v in zip(a, b):
        assert torch.equal(u, v)
