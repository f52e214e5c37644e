"""CPU checks of the exact-arithmetic attention inputs (tests/attn_exact_util.py): every case that the GPU
tests launch meets its exactness conditions and reaches the edges it claims.  No GPU, and nothing of the
product package."""
import pytest
import torch

import attn_exact_util as U


def _noncausal(d):
    seen = {}
    for form in ("nw4", "nw8", "nw8_stag", "qb2", "auto"):
        if form != "auto" and d not in U.FORM_DIMS[form]:
            continue
        for family, B, H, nq, nk, negative, _ in U.noncausal_specs(form, d):
            seen[(family, B, H, nq, nk, negative)] = U.rows_of(form, d)
    return [(U.get_case(f, B, H, nq, nk, d, False, neg), rows) for (f, B, H, nq, nk, neg), rows in seen.items()]


def _causal(d):
    return [U.get_case(f, B, H, nq, nk, d, True) for f, B, H, nq, nk, _ in U.causal_specs(d, d in (40, 64, 80))]


def _check_reference(c):
    """float32 and float64 agree: the same numerator and denominator exactly (weighted: every partial sum is
    exact), the same fp16 for the one-hot family, and fp16 outputs at most 1 ulp apart for the weighted one
    (two roundings of the quotient against one)."""
    n32, d32, o32 = U.reference(c, torch.float32)
    n64, d64, o64 = U.reference(c, torch.float64)
    assert torch.equal(o64.half(), c.ref)
    if c.family == "onehot":
        assert torch.equal(o32.half(), c.ref), c.name
        assert c.min_gap >= U.GAP, c.name
    else:
        assert torch.equal(n32.double(), n64) and torch.equal(d32.double(), d64), c.name
        assert U.ulp_diff(o32.half(), c.ref) <= 1, c.name
        assert c.nk * 4 ** c.spread * U.VMAX < 2 ** 24 and c.spread < 8, c.name


@pytest.mark.parametrize("d", U.ALL_DIMS)
def test_noncausal_cases_meet_their_conditions(d):
    """Every case builds (Case.__init__ raises InexactCase otherwise: integral fp16 inputs, the intended
    winner wins by >= 64, negative winners <= -64, nk * 4^S * Vmax < 2^24 with S < 8) and the references
    agree.  Every Q and K column is used by some row, and every 32-row wave of every workgroup holds a row
    that wins in tile 0 (its running max never moves again) and one that wins later (a forced rescale)."""
    cases = _noncausal(d)
    assert len(cases) >= 12
    for c, rows in cases:
        _check_reference(c)
        assert c.q.dtype == torch.float16 and c.k.dtype == torch.float16 and c.v.dtype == torch.float16
        if c.nq * 2 >= d:                                  # 2-3 entries per row cannot cover d columns in 5 rows
            assert (c.q != 0).any(dim=1).all(), (c.name, "an unused Q column")
        assert (c.k != 0).any(dim=1).all(), (c.name, "an unused K column")
        if c.family == "onehot":
            assert c.v.max().item() < 2048
            tile = c.win // U.KT                           # [B, H, nq]
            assert tile.max().item() == c.ntiles - 1
            if c.nk % U.KT == 1:
                assert (c.win == c.nk - 1).any(), (c.name, "the 1-key tail never wins")
            if c.ntiles > 1:
                for w0 in range(0, c.nq, 32):
                    t = tile[:, :, w0:w0 + 32]
                    if t.shape[-1] < 2:
                        continue
                    assert ((t == 0).any(-1) & (t > 0).any(-1)).all(), (c.name, rows, "wave at row", w0)
    # the shapes reach a full workgroup with lag waves, then two full waves, a 5-row wave and empty waves
    nqs = {c.nq for c, _ in cases}
    assert 128 + 69 in nqs and 5 in nqs and (d not in U.FORM_DIMS["nw8"] or 256 + 69 in nqs)
    assert {c.nk for c, _ in cases} >= set(U.NKS)
    assert any(c.negative and c.nk % U.KT for c, _ in cases)


@pytest.mark.parametrize("d", (16, 32, 40, 64, 80, 96, 128, 160))
def test_causal_cases_meet_their_conditions(d):
    """f(i) <= i; every trap lies strictly above the diagonal and scores >= 64 above the row's winner, so
    only the mask keeps it out; diagonal rows (both traps) include i = 63, 64, 65 and the first and last
    row of every workgroup."""
    for c in _causal(d):
        _check_reference(c)
        if c.family != "onehot":
            continue
        i = torch.arange(c.nq).view(1, 1, -1)
        assert (c.win <= i).all() and (c.win < c.nk).all()
        margins = U.trap_margins(c)
        assert margins and all(dist > 0 and m >= U.GAP for dist, m in margins), c.name
        traps = set(c.traps)
        for r in {0, 63, 64, 65, 127, 128, 255, 256, c.nq - 1}:
            if r >= c.nq:
                continue
            assert c.kinds[r] == "diag", (c.name, r)
            if r + 1 < c.nk:
                assert (r, r + 1) in traps
            nxt = U.KT * (r // U.KT + 1)
            if nxt < c.nk:
                assert (r, nxt) in traps
        assert "code" in c.kinds and any(int(c.win[0, 0, r]) < r for r in range(c.nq) if c.kinds[r] == "code")


def test_inexact_case_is_a_test_error(monkeypatch):
    """Inputs that break a condition raise InexactCase while the case is built."""
    with pytest.raises(U.InexactCase, match="no room"):
        U.Case("onehot", 1, 1, 8, 129, 8, negative=True)          # 8 bits + the constant column in 8 columns
    monkeypatch.setattr(U, "VMAX", 4096)
    with pytest.raises(U.InexactCase, match="limit|fp32 integers"):
        U.Case("weighted", 1, 1, 64, 257, 40)
    monkeypatch.setattr(U, "VMAX", 15)
    monkeypatch.setattr(U, "GAP", 16)                             # amplitudes sized for a gap of 16 only
    real = U.Case.check_conditions

    def strict(self):
        monkeypatch.setattr(U, "GAP", 64)
        real(self)
    monkeypatch.setattr(U.Case, "check_conditions", strict)
    with pytest.raises(U.InexactCase, match="gap below"):
        U.Case("onehot", 1, 1, 64, 129, 16)


@pytest.mark.parametrize("C,D", U.XATTN_SHAPES)
def test_cross_attention_cases_are_exact(C, D):
    """XCase raises InexactCase unless t Wq^T is the one-hot family's Q and every intermediate is an integer
    within 2048; Wq / Wo are non-involutive signed permutations, so a transposed weight is another matrix."""
    wq, wo, bias = U.xattn_weights(C)
    for w in (wq, wo):
        assert (w.abs().sum(0) == 1).all() and (w.abs().sum(1) == 1).all() and not torch.equal(w, w.T)
        assert (w < 0).any() and (w > 0).any() and not torch.equal(w @ w, torch.eye(C, dtype=w.dtype))
    assert torch.equal(bias, bias.round()) and bias.abs().max().item() <= 8
    for n_img in U.XATTN_N:
        for nk in U.XATTN_NK:
            for negative in ((False, True) if nk < 80 else (False,)):
                c = U.XCase(2, n_img, C, D, nk, negative)
                assert c.ref.dtype == torch.float16 and c.ref.float().abs().max().item() > 256
                assert (c.win < nk).all()


def test_form_table():
    """The (form, d) table the GPU tests assert, against literals."""
    assert U.expected_info("auto", 40) == dict(form="nw8", dqk=48, dv=64, waves=8, qblocks=1, stagger=0, seed_col=40,
                                               causal=0)
    assert U.expected_info("auto", 64)["stagger"] == 1 and U.expected_info("auto", 80)["stagger"] == 1
    assert U.expected_info("auto", 160)["waves"] == 4 and U.expected_info("auto", 32)["waves"] == 4
    assert U.expected_info("nw8_stag", 40, causal=True) == dict(form="nw8_stag", dqk=48, dv=64, waves=8, qblocks=1,
                                                                stagger=0, seed_col=0, causal=1)
    assert U.rows_of("qb2", 48) == 256 and U.rows_of("nw4", 160) == 128
    assert U.SCALE * 1.4426950408889634 == pytest.approx(1.0, abs=2.0 ** -23)
