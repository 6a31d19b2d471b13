"""CPU: the two backbone switches (modules.S1_BACKBONE / S2_BACKBONE): the spellings their environment variables
accept, True / False as all / none of the marked convs, a layer set routing exactly its layers (through the layer
index DetectionModel gives the marked stride-2 convs and Conv.forward_fuse hands on), and the defaults DESIGN.md
section 21 states."""
import re
from pathlib import Path

import pytest
import torch

from yolosod_amd.nn import modules as M
from yolosod_amd.nn.tasks import DetectionModel

CFG = "yolov12-sod-fusion-v5-simple.yaml"


def test_environment_spellings():
    L = M.S2_BACKBONE_LAYERS
    assert L == (7, 10)
    assert M._backbone_switch("0", L) is False and M._backbone_switch("1", L) is True
    assert M._backbone_switch("7", L) == frozenset({7}) and M._backbone_switch("10", L) == frozenset({10})
    assert M._backbone_switch("7,10", L) is True and M._backbone_switch(" 10,7 ", L) is True  # every layer: all
    for bad in ("", "yes", "2", "7,", "7,8", "3", "-1"):
        with pytest.raises(ValueError):
            M._backbone_switch(bad, L)
    # the stride-1 switch is all or none
    assert M._backbone_switch("0") is False and M._backbone_switch("1") is True
    for bad in ("3", "3,6,8,11", "on"):
        with pytest.raises(ValueError):
            M._backbone_switch(bad)


def test_true_false_mean_all_or_none(monkeypatch):
    monkeypatch.setattr(M, "S2_BACKBONE", True)
    assert M._s2_on("backbone") is True and all(M._s2_on("backbone", i) for i in (7, 10, 99))
    monkeypatch.setattr(M, "S2_BACKBONE", False)
    assert M._s2_on("backbone") is False and not any(M._s2_on("backbone", i) for i in (7, 10, 99))
    monkeypatch.setattr(M, "S2_NECK", True)
    assert M._s2_on(True) and M._s2_on(True, 7) and not M._s2_on(False, 7)  # the neck's mark ignores the layer
    monkeypatch.setattr(M, "S1_BACKBONE", True)
    assert M._s1_on("backbone")
    monkeypatch.setattr(M, "S1_BACKBONE", False)
    assert not M._s1_on("backbone")


@pytest.mark.parametrize("layers", [{7}, {10}])
def test_layer_set_routes_exactly_its_layers(layers, monkeypatch):
    m = DetectionModel(CFG)
    marked = {i: layer for i, layer in enumerate(m.model) if getattr(layer, "s2_backbone", False)}
    assert sorted(marked) == [7, 10] and all(layer.layer == i for i, layer in marked.items())
    assert all(c.layer is None for c in m.modules() if isinstance(c, M.Conv) and not c.s2_backbone)
    monkeypatch.setattr(M, "S2_BACKBONE", frozenset(layers))
    assert M._s2_on("backbone") == frozenset(layers)  # asked without a layer: the switch itself
    assert {i for i in marked if M._s2_on("backbone", i)} == layers
    # forward_fuse hands conv_epilogue the mark and the layer index
    seen = []

    def spy(conv, act_code, x, *a):
        seen.append((a[6], a[9]))  # s2, layer
        return x

    monkeypatch.setattr(M, "conv_epilogue", spy)
    x = torch.zeros(1)
    for i, layer in marked.items():
        layer.forward_fuse(x)
    assert seen == [("backbone", 7), ("backbone", 10)]
    assert [M._s2_on(*s) for s in seen] == [7 in layers, 10 in layers]


def test_defaults_are_those_of_design_21():
    assert (M.S1_BACKBONE_DEFAULT, M.S2_BACKBONE_DEFAULT) == ("1", "10")
    assert M._backbone_switch(M.S1_BACKBONE_DEFAULT) is True
    assert M._backbone_switch(M.S2_BACKBONE_DEFAULT, M.S2_BACKBONE_LAYERS) == frozenset({10})
    design = (Path(__file__).resolve().parents[1] / "DESIGN.md").read_text()
    sec = design[design.index("\n## 21."):]
    m = re.search(r"`YOLOSOD_S1_BACKBONE` defaults to (\S+) and `YOLOSOD_S2_BACKBONE` to (\S+?)[.*]", sec)
    assert m and (m.group(1), m.group(2)) == (M.S1_BACKBONE_DEFAULT, M.S2_BACKBONE_DEFAULT), m
