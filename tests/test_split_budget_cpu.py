"""CPU: the split conv kernels' error budget (tests/split_budget.py) has teeth. The bit-exact emulation of the kernels'
arithmetic keeps |y - ref64| <= 8 E32 + 1.1 F at every scale, flat and with per-channel scales of 2^-10 .. 2^2, and at
scales >= 2^-6 every mutant that loses one term (a whole low-term product, the subnormal low terms, one tap's or one
32-channel chunk's low terms) breaks it somewhere. Scale 1e-3 is budget-only: there the activations' low terms are at
the floor themselves, so dropping them is not an error the method promises to avoid.
tests/test_gpu_split_budget.py holds the kernels to the same budget."""
import pytest
import torch

import split_budget as sb


@pytest.fixture(autouse=True)
def _keep_denormals():
    """The emulation needs fp16's subnormals and fp32's; make sure no earlier test left the CPU flushing them."""
    torch.set_flush_denormal(False)
    yield


@pytest.mark.parametrize("case", sb.CASES, ids=lambda c: "x".join(map(str, c)))
def test_emulation_keeps_the_budget_and_every_mutant_breaks_it(case):
    k, stride = case[5], case[6]
    for s, wide in sb.variants():
        x, w, b = sb.make_case(*case, s, wide)
        ref64, lim = sb.budget(x, w, b, k, stride)
        assert ref64.shape == lim.shape and bool((lim > 0).all())
        r = sb.worst_ratio(sb.emulate(x, w, b, k, stride), ref64, lim)
        print(f"{case} s={s:.3g} wide={wide}: split {r:.3f}")
        assert r <= 1.0, (case, s, wide, r)
        if s not in sb.MUTANT_SCALES:
            continue
        for m in sb.MUTANTS:
            rm = sb.worst_ratio(sb.emulate(x, w, b, k, stride, mutant=m), ref64, lim)
            print(f"{case} s={s:.3g} wide={wide}: {m} {rm:.3f}")
            assert rm > 1.0, (case, s, wide, m, rm)


def test_make_case_is_deterministic_and_the_bias_follows_the_signal():
    case = sb.CASES[3]
    a, b = sb.make_case(*case, 2.0 ** -6, True), sb.make_case(*case, 2.0 ** -6, True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    x, _, bias = a
    assert float(bias.abs().max()) < float(x.abs().mean())


def test_gates_enter_the_budget_in_the_kernel_order():
    """x_eff = (x * gate_c) * gate_p in fp32; the floor follows the gated activations."""
    case = sb.CASES[3]
    x, w, b = sb.make_case(*case, 2.0 ** -6, False)
    g = torch.Generator().manual_seed(1)
    gc, gp = torch.rand(case[0], case[1], generator=g), torch.rand(case[0], case[3], case[4], generator=g)
    ref_g, lim_g = sb.budget(x, w, b, 3, 2, gate_c=gc, gate_p=gp)
    ref_e, lim_e = sb.budget((x * gc[:, :, None, None]) * gp[:, None], w, b, 3, 2)
    assert torch.equal(ref_g, ref_e) and torch.equal(lim_g, lim_e)
    r = sb.worst_ratio(sb.emulate(sb.gated(x, gc, gp), w, b, 3, 2), ref_g, lim_g)
    assert r <= 1.0, r
