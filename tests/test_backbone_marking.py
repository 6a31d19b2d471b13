"""CPU: DetectionModel marks the C2f Bottleneck 3x3 / stride-1 convs for the stride-1 fp16-split kernel - the neck's
with ``s1`` (modules.S1_NECK), the backbone's with ``s1_backbone`` (modules.S1_BACKBONE) - and nothing else."""
from yolosod_amd.nn import modules as M
from yolosod_amd.nn.tasks import DetectionModel


def test_c2f_bottleneck_convs_are_marked():
    m = DetectionModel("yolov12-sod-fusion-v5-simple.yaml")
    nb = len(m.yaml["backbone"])
    marked = {id(c) for c in m.modules() if isinstance(c, M.Conv) and (c.s1 or c.s1_backbone)}
    want_backbone, want_neck = [], []
    for i, layer in enumerate(m.model):
        if isinstance(layer, M.C2f):
            for bt in layer.m:
                (want_backbone if i < nb else want_neck).extend([bt.cv1, bt.cv2])
    assert [i for i, layer in enumerate(m.model) if isinstance(layer, M.C2f) and i < nb] == [3, 6, 8, 11]
    assert len(want_backbone) == 10 and len(want_neck) == 12
    assert all(c.s1_backbone and not c.s1 and c.s1_mark() == "backbone" for c in want_backbone)
    assert all(c.s1 is True and not c.s1_backbone and c.s1_mark() is True for c in want_neck)
    assert len(marked) == 22  # no other Conv carries the mark (the C2fs' own 1x1 convs, the stride-2 convs, Detect)
    for c in want_backbone + want_neck:
        assert c.conv.kernel_size == (3, 3) and c.conv.stride == (1, 1) and c.conv.groups == 1


def test_gate_free_backbone_stride2_convs_are_marked():
    """Layers 7 and 10; not the stem, not the consumers of SE L1 / CBAM L4 (they apply those gates), and the neck's
    stride-2 convs keep their own mark."""
    m = DetectionModel("yolov12-sod-fusion-v5-simple.yaml")
    assert [i for i, layer in enumerate(m.model) if getattr(layer, "s2_backbone", False)] == [7, 10]
    assert [i for i, layer in enumerate(m.model) if getattr(layer, "s2", False)] == [29, 33, 36]
    assert M._s2_on("backbone") == M.S2_BACKBONE and M._s2_on(True) == M.S2_NECK and not M._s2_on(False)


def test_switches_select_by_mark(monkeypatch):
    monkeypatch.setattr(M, "S1_NECK", True)
    monkeypatch.setattr(M, "S1_BACKBONE", False)
    assert M._s1_on(True) and not M._s1_on("backbone") and not M._s1_on(False)
    monkeypatch.setattr(M, "S1_NECK", False)
    monkeypatch.setattr(M, "S1_BACKBONE", True)
    assert not M._s1_on(True) and M._s1_on("backbone") and not M._s1_on(False)
