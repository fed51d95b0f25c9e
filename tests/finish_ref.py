"""fp64 numpy references of the spectral-norm power iteration, the weight-gradient un-folds and the spectral-norm finish
(csrc/spectral.hip), in the layouts include/gim_hip.h documents.  TEST INFRASTRUCTURE ONLY: needs neither torch nor the library;
tests/test_finish_ref_host.py pins it to oracle.gim_oracle.sn_weight and to fp64 autograd, tests/test_gpu_finish_kernels.py holds
the kernels to it.

Every function returns, beside its value, the same expression with absolute values taken term by term: the scale of the a-priori
rounding bound |got - ref| <= gamma(m) * scale of an fp32 evaluation with at most m operations on the path to an element."""
import numpy as np

EPS = 1e-12           # torch.nn.utils.spectral_norm's eps
U32 = 2.0 ** -24      # unit roundoff of fp32


def gamma(m):
    """gamma_m = m u / (1 - m u): the relative error bound of m fp32 operations in a row (Higham, Accuracy and Stability, 3.1)."""
    return m * U32 / (1.0 - m * U32)


def weight_mat(W):
    """torch's weight_mat [Cout][Cin*K*K] (column q = ci*T + tap) of W [Cout][K][K][Cin] (memory order)."""
    W = np.asarray(W, dtype=np.float64)
    assert W.ndim == 4 and W.shape[1] == W.shape[2], W.shape
    return W.transpose(0, 3, 1, 2).reshape(W.shape[0], -1)


def v_mem(v, Cin, K):
    """v (reference order (ci, kh, kw)) as [K][K][Cin], the order of a weight row in memory."""
    return np.asarray(v, dtype=np.float64).reshape(Cin, K, K).transpose(1, 2, 0)


def _normalize(a):
    return a / max(np.linalg.norm(a), EPS)      # F.normalize(a, dim=0, eps)


def power_iteration(W, u, v, training, degenerate_ok=False):
    """One round of torch.nn.utils.spectral_norm (n_power_iterations = 1, eps = 1e-12, dim = 0) on W [Cout][K][K][Cin] with
    v in the reference's (ci, kh, kw) order:  training: v <- normalize(W^T u), u <- normalize(W v);  sigma = u^T W v.
    -> (sigma, u, v, S) with S = sum |u_i W_ij v_j|, the cancellation-free scale of sigma.
    A normalisation of a vector shorter than 1e-2 is refused (the comparison would be ill-conditioned) unless degenerate_ok."""
    M = weight_mat(W)
    u, v = np.asarray(u, dtype=np.float64).copy(), np.asarray(v, dtype=np.float64).copy()
    assert u.shape == (M.shape[0],) and v.shape == (M.shape[1],), (u.shape, v.shape, M.shape)
    if training:
        a = M.T @ u
        assert degenerate_ok or np.linalg.norm(a) > 1e-2, "|W^T u| = %.3e" % np.linalg.norm(a)
        v = _normalize(a)
        t = M @ v
        assert degenerate_ok or np.linalg.norm(t) > 1e-2, "|W v| = %.3e" % np.linalg.norm(t)
        u = _normalize(t)
    sigma = float(u @ (M @ v))
    S = float(np.abs(u) @ (np.abs(M) @ np.abs(v)))
    return sigma, u, v, S


def normalize_with_bound(a, a_abs, m_sum, m_norm):
    """n = a / |a| and the bound of an fp32 evaluation whose a_j carries |error| <= gamma(m_sum) * a_abs_j (a sum of products, a_abs
    the sum of their absolute values) and whose norm and division take m_norm further operations:
        |n^_j - n_j| <= gamma(m_sum) a_abs_j / |a|  +  |n_j| (gamma(m_sum) |a_abs| / |a| + gamma(m_norm))
    (first order in u; the first term is the element's own error, the bracket the relative error of the computed norm - by the
    triangle inequality at most |error vector| / |a| - plus the rounding of sum of squares, sqrt, reciprocal and product)."""
    nrm = np.linalg.norm(a)
    n = a / nrm
    bound = gamma(m_sum) * a_abs / nrm + np.abs(n) * (gamma(m_sum) * np.linalg.norm(a_abs) / nrm + gamma(m_norm))
    return n, bound


def power_iteration_stages(W, u_in, v_got, u_got):
    """The two stages of a TRAINING round one at a time, each from what the device really fed it, so that each bound covers
    one stage's rounding only:  v against normalize(W^T u_in);  u against normalize(W v_got);  sigma against u_got^T W v_got.
    -> (v_ref, v_bound, u_ref, u_bound, sigma_ref, S).
    Operation counts (upper bounds: the kernels' chains are shorter): a column of W^T u is Cout products and Cout + 8 additions
    (eight row chunks), m_sum = 2 Cout + 8; a row of W v is K products and K additions (lane loop and wave tree), m_sum = 2 K;
    a norm is L squares, L additions, sqrt, reciprocal and the final product, m_norm = 2 L + 3."""
    M = weight_mat(W)
    Cout, K = M.shape
    u_in, v_got, u_got = (np.asarray(t, dtype=np.float64) for t in (u_in, v_got, u_got))
    v_ref, v_bound = normalize_with_bound(M.T @ u_in, np.abs(M).T @ np.abs(u_in), 2 * Cout + 8, 2 * K + 3)
    u_ref, u_bound = normalize_with_bound(M @ v_got, np.abs(M) @ np.abs(v_got), 2 * K, 2 * Cout + 3)
    sigma_ref = float(u_got @ (M @ v_got))
    S = float(np.abs(u_got) @ (np.abs(M) @ np.abs(v_got)))
    return v_ref, v_bound, u_ref, u_bound, sigma_ref, S


def row_pad(K, Cin):
    """Floats per tap row of the row-padded slot of gim_conv2d_wgrad_rows_acc: K * Cin rounded up to 16."""
    return (K * Cin + 15) // 16 * 16


def src_size(Cout, Cin, K, fold):
    """Floats of the source slot / slab of a weight gradient in fold code `fold`."""
    return {0: Cout * K * K * Cin, 1: Cout * (K + 1) ** 2 * Cin, 2: Cin * (K + 1) ** 2 * Cout, 3: Cout * K * row_pad(K, Cin)}[fold]


def unfold(src, Cout, Cin, K, fold):
    """The raw gradient `src` (flat) as dW [Cout][K][K][Cin], and the same expression over |src|:
       0: identity;
       1: src = dF [Cout][K+1][K+1][Cin]:  0.25 * sum_{dh,dw in {0,1}} dF[co][kh+dh][kw+dw][ci]   (pool form);
       2: src = G  [Cin][K+1][K+1][Cout] with dF[co][a][b][ci] = G[ci][K-a][K-b][co]: the same sum without the factor (sub-pixel form);
       3: src = [Cout][K][K*Cin rounded up to 16]: the un-padded rows."""
    src = np.asarray(src, dtype=np.float64).reshape(-1)
    assert src.size == src_size(Cout, Cin, K, fold), (src.size, Cout, Cin, K, fold)
    KF = K + 1
    if fold == 0:
        g = src.reshape(Cout, K, K, Cin)
        return g.copy(), np.abs(g)
    if fold == 3:
        g = src.reshape(Cout, K, row_pad(K, Cin))[:, :, :K * Cin].reshape(Cout, K, K, Cin)
        return g.copy(), np.abs(g)
    if fold == 1:
        dF = src.reshape(Cout, KF, KF, Cin)
    elif fold == 2:
        dF = src.reshape(Cin, KF, KF, Cout)[:, ::-1, ::-1, :].transpose(3, 1, 2, 0)
    else:
        raise ValueError("fold code %r" % (fold,))
    g, ga = np.zeros((Cout, K, K, Cin)), np.zeros((Cout, K, K, Cin))
    for dh in (0, 1):
        for dw in (0, 1):
            g += dF[:, dh:dh + K, dw:dw + K, :]
            ga += np.abs(dF[:, dh:dh + K, dw:dw + K, :])
    f = 0.25 if fold == 1 else 1.0
    return f * g, f * ga


def finish(g, W, sigma, u, v, g_abs=None):
    """dW = g / sigma - (<g, W> / sigma^2) u v^T (autograd of weight_orig / (u^T W v) with u, v constants) for g, W
    [Cout][K][K][Cin] and v in the reference's order, and its elementwise scale |g_i| / |sigma| + (sum |g W| / sigma^2) |u_co v_q|.
    g_abs: the sum of absolute values behind g where g itself is a sum (slabs, folds); |g| otherwise."""
    g, W = np.asarray(g, dtype=np.float64), np.asarray(W, dtype=np.float64)
    Cout, K, _, Cin = W.shape
    assert g.shape == W.shape
    g_abs = np.abs(g) if g_abs is None else np.asarray(g_abs, dtype=np.float64)
    sigma = float(sigma)
    uv = np.asarray(u, dtype=np.float64)[:, None, None, None] * v_mem(v, Cin, K)[None]
    dw = g / sigma - (np.sum(g * W) / sigma ** 2) * uv
    scale = g_abs / abs(sigma) + (np.sum(g_abs * np.abs(W)) / sigma ** 2) * np.abs(uv)
    return dw, scale
