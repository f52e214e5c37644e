"""The exact token-linear cases (tests/token_exact_util.py) checked on the CPU: the row counts reach the
branches of the persistent kernel they claim for any CU count, the exactness conditions hold, each
InexactCase condition fires on a deliberately bad input, and the float64 reference reproduces itself in
float32 under a permuted summation order."""
import copy

import pytest
import torch

import token_exact_util as T

CUS = (256, 304, 64, 8)


@pytest.mark.parametrize("G", CUS)
def test_row_counts_reach_the_claimed_branches(G):
    assert [T.rows_of(k, G) for k in ("7", "32", "33", "1000")] == [7, 32, 33, 1000]
    grid, nblk, its, last = T.walk(T.rows_of("it1", G), G)
    assert grid == G and nblk == G + 2 and max(its) == 1 and its.count(1) == 2 and last == 8
    grid, nblk, its, last = T.walk(T.rows_of("it3", G), G)
    assert grid == G and nblk == 3 * G + 6 and max(its) == 3 and last == 9
    assert [b % grid for b in range(nblk) if its[b] == 3] == [0, 1, 2, 3, 4, 5]       # the ragged block is workgroup 5's fourth
    assert 3 % T.STAGES == 0                                                         # the ring is back in stage 0
    if G == 256:
        assert T.rows_of("it3", G) == 24745
    for k, want in (("7", (1, 7)), ("32", (1, 32)), ("33", (2, 1)), ("1000", (32, 8))):
        _, nblk, _, last = T.walk(T.rows_of(k, G), G)
        assert (nblk, last) == want


@pytest.mark.parametrize("M", [7, 33, 1000, T.rows_of("it1", 64)])
def test_token_case_is_exact(M):
    c = T.token_case(M)
    for with_bias in (False, True):
        for with_res in (False, True):
            ref = T.token_ref(c, with_bias, with_res)
            assert ref.dtype == torch.float16 and ref.shape == (M, 320) and bool(torch.isfinite(ref).all())
            for seed in (1, 2):
                assert torch.equal(T.token_reference_f32(c, with_bias, with_res, seed), ref)
    x, w = c.x.double(), c.w.double()
    uniq = lambda v: torch.unique(v, dim=0).shape[0] == v.shape[0]
    assert uniq(x) and uniq(w) and uniq(w.T) and uniq(c.res.double())
    assert bool((w != 0).any(0).all()) and bool((w != 0).any(1).all())
    if M >= 33:
        # both roundings are real: rounding acc + b + res once differs somewhere from rounding twice
        acc = x @ w.T + c.b.double()
        assert acc.abs().max().item() > 2048
        once = (acc + c.res.double()).float().half()
        assert int((once != T.token_ref(c, True, True)).sum()) > 0
    assert torch.equal(T.token_case(7).x, T.token_case(33).x[:7])


def _bad(**kw):
    c = copy.copy(T.token_case(33))
    c.ref = {}
    for k, v in kw.items():
        setattr(c, k, v(getattr(c, k).clone()))
    return c


@pytest.mark.parametrize("what,kw", [
    ("not integral", dict(x=lambda v: v + 0.25)),
    ("partial sum can reach 2\\^24", dict(x=lambda v: v * 4096, w=lambda v: v * 4096)),
    ("acc \\+ b\\| reaches 65504", dict(b=lambda v: v + 70000)),
    ("acc \\+ b \\+ res\\| reaches 65504", dict(b=lambda v: v * 0 + 40000, res=lambda v: v * 0 + 30000)),
])
def test_inexact_inputs_are_test_errors(what, kw):
    with pytest.raises(T.InexactCase, match=what):
        T.token_reference(_bad(**kw), True, True)


def test_layer_norm_reference_is_float64():
    c = T.token_case(7)
    out = T.token_ref(c, True, False)
    g, b = torch.linspace(0.5, 1.5, 320), torch.linspace(-1, 1, 320)
    y = T.layer_norm_ref(out, g, b, 1e-5)
    assert y.dtype == torch.float64
    z = (out.double() - out.double().mean(1, keepdim=True)) / (out.double().var(1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    assert torch.allclose(y, z * g.double() + b.double(), rtol=1e-12, atol=1e-12)
    assert "workgroup 5 of 8, it 3" in T.token_where(T.rows_of("it3", 8), 8)(T.rows_of("it3", 8) - 1, 100)
