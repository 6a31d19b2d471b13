"""CPU: the backbone's wide-1x1 switch (modules.N1_BACKBONE): the spellings YOLOSOD_N1_BACKBONE accepts, True / False
as all / none of the marked convs, a layer set routing exactly its layers, which convs of the paper YAML carry the mark
(cv1 / cv2 of the C2fs L6 / L8 / L11 and of SPPF L13), and that none of them carries the neck's ``n1``."""
import pytest
import torch

from yolosod_amd.nn import modules as M
from yolosod_amd.nn.tasks import DetectionModel

CFG = "yolov12-sod-fusion-v5-simple.yaml"
# (layer, conv, Cin, Cout) of the eight marked convs
MARKED = [(6, "cv1", 128, 128), (6, "cv2", 256, 128), (8, "cv1", 256, 256), (8, "cv2", 384, 256),
          (11, "cv1", 512, 512), (11, "cv2", 768, 512), (13, "cv1", 512, 256), (13, "cv2", 1024, 512)]


def test_environment_spellings():
    L = M.N1_BACKBONE_LAYERS
    assert L == (6, 8, 11, 13)
    assert M._backbone_switch("0", L) is False and M._backbone_switch("1", L) is True
    assert M._backbone_switch("6", L) == frozenset({6})
    assert M._backbone_switch("8,13", L) == frozenset({8, 13}) and M._backbone_switch(" 13, 8 ", L) == frozenset({8, 13})
    assert M._backbone_switch("6,8,11,13", L) is True  # every layer: all
    for bad in ("", "on", "3", "7", "6,", "6,7", "6;8", "-1", "2"):
        with pytest.raises(ValueError):
            M._backbone_switch(bad, L)
    M._backbone_switch(M.N1_BACKBONE_DEFAULT, L)  # the shipped default is one of the spellings


def test_true_false_mean_all_or_none(monkeypatch):
    monkeypatch.setattr(M, "N1_BACKBONE", True)
    assert M._n1_on("backbone") is True and all(M._n1_on("backbone", i) for i in (6, 8, 11, 13, 99))
    monkeypatch.setattr(M, "N1_BACKBONE", False)
    assert M._n1_on("backbone") is False and not any(M._n1_on("backbone", i) for i in (6, 8, 11, 13))
    monkeypatch.setattr(M, "N1_NECK", True)
    assert M._n1_on(True) and M._n1_on(True, 6) and not M._n1_on(False, 6)  # the neck's mark ignores the layer
    monkeypatch.setattr(M, "N1_NECK", False)
    monkeypatch.setattr(M, "N1_BACKBONE", True)
    assert not M._n1_on(True) and M._n1_on("backbone", 6)  # the two switches are independent


def test_paper_yaml_marks():
    m = DetectionModel(CFG)
    got = []
    for i, layer in enumerate(m.model):
        for name in ("cv1", "cv2"):
            cv = getattr(layer, name, None)
            if isinstance(cv, M.Conv) and cv.n1_backbone:
                got.append((i, name, cv.conv.in_channels, cv.conv.out_channels))
                assert cv.n1_layer == i and cv.n1 is False and cv.conv.kernel_size == (1, 1)
    assert got == MARKED
    marked = [c for c in m.modules() if isinstance(c, M.Conv) and c.n1_backbone]
    assert len(marked) == 8
    # nothing else carries the mark or a layer of this kind; the neck's convs keep n1 and nothing of the backbone has it
    assert all(c.n1_layer is None for c in m.modules() if isinstance(c, M.Conv) and not c.n1_backbone)
    nb = len(m.yaml["backbone"])
    for i, layer in enumerate(m.model):
        n1 = [c for c in layer.modules() if isinstance(c, M.Conv) and c.n1]
        assert not n1 if i < nb else True, i
    assert sum(1 for c in m.modules() if isinstance(c, M.Conv) and c.n1) >= 8


@pytest.mark.parametrize("layers", [{6}, {8, 13}, {11}])
def test_layer_set_routes_exactly_its_layers(layers, monkeypatch):
    m = DetectionModel(CFG)
    monkeypatch.setattr(M, "N1_BACKBONE", frozenset(layers))
    seen = []

    def spy(conv, act_code, x, *a):
        seen.append((a[8], a[9]))  # n1, layer
        return x

    monkeypatch.setattr(M, "conv_epilogue", spy)
    x = torch.zeros(1)
    for i, name, _, _ in MARKED:
        getattr(m.model[i], name).forward_fuse(x)
    assert seen == [("backbone", i) for i, _, _, _ in MARKED]
    assert [M._n1_on(*s) for s in seen] == [i in layers for i, _, _, _ in MARKED]
