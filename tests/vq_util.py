"""Inputs of the vector-quantiser fixtures, regenerated from seeds (shared by
tests/golden/make_golden_vq.py and the tests): codebooks and latents are N(0, 1) fp32 from numpy's
PCG64, so the fixtures hold indices, gaps and outputs only.

The reference's default codebook init, U(±1/n_e), puts every code within 1e-4 of zero and makes
almost every row a near-tie; randn data keeps the argmin well-conditioned."""
import numpy as np

# (n_e, e_dim, B, H, W) of the kernel-against-reference cases
KERNEL_CASES = [(8192, 3, 2, 16, 16), (256, 4, 1, 8, 8), (16384, 8, 1, 8, 8), (512, 64, 4, 16, 16),
                (1000, 20, 1, 7, 11), (1024, 256, 1, 4, 4), (5, 1, 1, 1, 1), (1, 3, 1, 2, 2)]
GAP_MIN = 1e-5          # rows whose relative fp64 gap is below this are near-ties
NEAR_TIE_CAP = 0.01     # at most 1 % of a case's rows


def case_tag(case):
    return "n{}_d{}_b{}_h{}_w{}".format(*case)


def case_seed(case):
    n, d, b, h, w = case
    return 1000003 * n + 1009 * d + 101 * b + 7 * h + w


def randn(seed, *shape):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal(shape, dtype=np.float32)


def case_data(case):
    """(codebook [n_e, e_dim], z [B, e_dim, H, W]) fp32 numpy."""
    n, d, b, h, w = case
    s = case_seed(case)
    return randn(s, n, d), randn(s + 1, b, d, h, w)


def rows_of(z):
    """NCHW → [B·H·W, C] (the reference's ``b c h w -> b h w c`` flattening)."""
    return np.ascontiguousarray(np.transpose(z, (0, 2, 3, 1))).reshape(-1, z.shape[1])


def dist64(z, codebook):
    """fp64 squared distances [M, n_e] of the rows of NCHW ``z`` to every code."""
    r = rows_of(z).astype(np.float64)
    e = codebook.astype(np.float64)
    return (r * r).sum(1)[:, None] + (e * e).sum(1)[None, :] - 2.0 * r @ e.T


def rel_gap(z, codebook, idx=None):
    """Per row: (second-best − best fp64 distance) / (‖z‖² + ‖e_best‖²); inf when n_e = 1.
    ``best`` is the fp64 argmin, or ``idx`` when given."""
    d = dist64(z, codebook)
    m = np.arange(d.shape[0])
    best = d.argmin(1) if idx is None else np.asarray(idx).reshape(-1)
    dbest = d[m, best]
    if d.shape[1] == 1:
        return np.full(d.shape[0], np.inf)
    d2 = d.copy()
    d2[m, best] = np.inf
    second = d2.min(1)
    r = rows_of(z).astype(np.float64)
    e = codebook.astype(np.float64)[best]
    return (second - dbest) / ((r * r).sum(1) + (e * e).sum(1))


def straight_through(z, codebook, idx):
    """The reference's z + (e − z), two fp32 roundings, NCHW."""
    b, c, h, w = z.shape
    e = codebook[np.asarray(idx).reshape(-1)].reshape(b, h, w, c).transpose(0, 3, 1, 2)
    return (z + (e - z).astype(np.float32)).astype(np.float32)
