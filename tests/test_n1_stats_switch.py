"""CPU: the switch of the neck's gate-feeding wide 1x1 convs (modules.N1_STATS): the spellings YOLOSOD_N1_STATS
accepts, True / False as all / none of the marked convs, a layer set routing exactly its layers, which convs of the
paper YAML carry the mark (cv2 of the C2fs L17 / L22 / L31) and that it lives in an attribute of its own
(``n1_stats_layer``: neither ``layer`` nor ``n1_layer``)."""
import pytest
import torch

from yolosod_amd.nn import modules as M
from yolosod_amd.nn.tasks import DetectionModel

CFG = "yolov12-sod-fusion-v5-simple.yaml"
MARKED = [(17, 384, 256, "summax"), (22, 192, 128, "sum"), (31, 192, 128, "capool")]


def test_environment_spellings_and_default():
    L = M.N1_STATS_LAYERS
    assert L == (17, 22, 31)
    assert M._backbone_switch("0", L) is False and M._backbone_switch("1", L) is True
    assert M._backbone_switch("17", L) == frozenset({17})
    assert M._backbone_switch("22,31", L) == frozenset({22, 31}) and M._backbone_switch(" 31, 22 ", L) == frozenset({22, 31})
    assert M._backbone_switch("17,22,31", L) is True  # every layer: all
    for bad in ("", "on", "6", "18", "17,", "17,18", "17;22", "-1", "2"):
        with pytest.raises(ValueError):
            M._backbone_switch(bad, L)
    assert M.N1_STATS_DEFAULT == "17,22,31"
    assert M._backbone_switch(M.N1_STATS_DEFAULT, L) is True


def test_true_false_mean_all_or_none(monkeypatch):
    monkeypatch.setattr(M, "N1_STATS", True)
    assert all(M._n1_stats_on(i) for i in (17, 22, 31, 99)) and not M._n1_stats_on(None)
    monkeypatch.setattr(M, "N1_STATS", False)
    assert not any(M._n1_stats_on(i) for i in (17, 22, 31, None))
    monkeypatch.setattr(M, "N1_STATS", frozenset({22}))
    assert [M._n1_stats_on(i) for i in (17, 22, 31, None)] == [False, True, False, False]


def test_paper_yaml_marks():
    m = DetectionModel(CFG)
    got = []
    for i, layer in enumerate(m.model):
        for c in layer.modules():
            if isinstance(c, M.Conv) and c.n1_stats_layer is not None:
                assert c is layer.cv2 and c.n1_stats_layer == i and c.n1 is True
                assert c.layer is None and c.n1_layer is None  # those two stay the stride-2 / backbone convs'
                got.append((i, c.conv.in_channels, c.conv.out_channels, c.emit_stats))
    assert got == MARKED
    # the mark is exactly "a neck n1 conv that feeds a gate"
    nb = len(m.yaml["backbone"])
    for i, layer in enumerate(m.model):
        for c in layer.modules():
            if isinstance(c, M.Conv):
                assert (c.n1_stats_layer is not None) == (i >= nb and c.n1 and c.emit_stats is not None), i


@pytest.mark.parametrize("layers", [True, False, {17}, {22, 31}])
def test_switch_routes_exactly_its_layers(layers, monkeypatch):
    m = DetectionModel(CFG)
    monkeypatch.setattr(M, "N1_STATS", layers if isinstance(layers, bool) else frozenset(layers))
    seen = []

    def spy(conv, act_code, x, *a):
        seen.append((a[2], a[8], a[10]))  # stats, n1, stats_layer
        return x

    monkeypatch.setattr(M, "conv_epilogue", spy)
    x = torch.zeros(1)
    for i, _, _, _ in MARKED:
        m.model[i].cv2.forward_fuse(x)
    assert seen == [(st, True, i) for i, _, _, st in MARKED]
    want = [layers if isinstance(layers, bool) else i in layers for i, _, _, _ in MARKED]
    assert [M._n1_stats_on(s[2]) for s in seen] == want
    # a neck n1 conv without a gate behind it hands no statistics layer over
    seen.clear()
    m.model[17].cv1.forward_fuse(x)
    assert seen == [(None, True, None)]
