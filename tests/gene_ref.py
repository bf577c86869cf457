"""TEST-ONLY: multi-gene SR fitness (csrc/sr_genes.hip, include/evogp_hip.h evogp_hip_sr_gene_fitness) restated in numpy float64.

``moments(Gv, y)`` takes the (pop, D, G) float32 gene values (``batch_forward``'s outputs; a malformed tree's are NaN) and the labels
and returns TWO-PASS float64 moments: mean (pop, G), C (pop, G, G), c (pop, G), the exact float32 min / max per gene, ``bad`` (some
value is not finite), ``kappa`` (pop, G) = 1 + max_d (g_jd - m_j)^2 / C_jj (the worst any pilot row can do to a shifted one-pass
sum; 1 where C_jj is 0) and the scalars ybar, syy_D.

``solve(mom)`` applies the rules to moments -- these or a kernel's own (``from_packed``):
    bad                                              loss and every coefficient NaN
    gene j with min == max, C_jj <= 0 or D == 1      flat: weight 0, no part in the solve
    the others in index order through LDL^T          d_j = C_jj - sum over kept k < j of l_jk^2 d_k; kept iff d_j > TAU C_jj
    kept set K                                       C_KK w = c_K; b0 = ybar - sum w_j m_j; loss = max(0, Syy/D - sum_K w_j c_j)
    a coefficient not finite as float32              all NaN
and returns loss (pop,), coef (pop, 1 + G), kept (pop, G) bool, ratio (pop, G) = d_j / C_jj (NaN for a flat gene) and cond (pop,), the
condition number of C_KK after diagonal scaling (1 for an empty K).

``borderline(ratio, lo, hi)``: some ratio of the tree lies in [lo, hi] -- the kept / dropped decision is then within reach of rounding."""
import numpy as np

TAU = 2.0 ** -30
GENES_MAX = 8


def n_moments(G):
    return G * (G + 5) // 2


def moments(Gv, y):
    Gv = np.asarray(Gv, np.float32)
    pop, D, G = Gv.shape
    y64 = np.asarray(y, np.float64).reshape(-1)
    assert y64.shape == (D,)
    ybar = y64.mean()
    v = y64 - ybar
    syy_D = float((v * v).sum() / D)
    with np.errstate(invalid="ignore", over="ignore"):
        bad = ~np.isfinite(Gv).all(axis=(1, 2))
        g = np.where(bad[:, None, None], 0.0, Gv.astype(np.float64))
        mean = g.sum(1) / D
        gc = g - mean[:, None, :]
        C = np.einsum("pdi,pdj->pij", gc, gc) / D
        c = np.einsum("pdi,d->pi", gc, v) / D
        var = np.einsum("pjj->pj", C)
        dev2 = (gc * gc).max(1)
        kappa = 1.0 + np.where(var > 0, dev2 / np.where(var > 0, var, 1.0), 0.0)
        mn, mx = np.where(bad[:, None], np.nan, Gv.min(1)), np.where(bad[:, None], np.nan, Gv.max(1))
    return dict(mean=mean, C=C, c=c, mn=mn, mx=mx, bad=bad, kappa=kappa, ybar=float(ybar), syy_D=syy_D, D=D)


def pack(mean, C, c):
    """(pop, G(G+5)/2): the means, the row-major upper triangle of C, then c -- the layout of the kernel's moments output"""
    G = mean.shape[1]
    iu = np.triu_indices(G)
    return np.concatenate([mean, C[:, iu[0], iu[1]], c], axis=1)


def from_packed(packed, G, mn, mx, bad, ybar, syy_D, D):
    """the moments dict ``solve`` reads, from a kernel's (pop, G(G+5)/2) rows and the exact per-gene min / max / bad of the reference"""
    packed = np.asarray(packed, np.float64)
    pop = packed.shape[0]
    iu = np.triu_indices(G)
    C = np.zeros((pop, G, G))
    C[:, iu[0], iu[1]] = packed[:, G:G + len(iu[0])]
    C[:, iu[1], iu[0]] = packed[:, G:G + len(iu[0])]
    return dict(mean=packed[:, :G], C=C, c=packed[:, G + len(iu[0]):], mn=mn, mx=mx, bad=bad, ybar=ybar, syy_D=syy_D, D=D)


def solve(mom, tau=TAU):
    mean, C, c = mom["mean"], mom["C"], mom["c"]
    pop, G = mean.shape
    D, ybar, syy_D = mom["D"], mom["ybar"], mom["syy_D"]
    loss, coef = np.full(pop, np.nan), np.full((pop, 1 + G), np.nan)
    kept_all, ratio, cond = np.zeros((pop, G), bool), np.full((pop, G), np.nan), np.ones(pop)
    for t in range(pop):
        if mom["bad"][t]:
            continue
        Lm, dd, kept = np.zeros((G, G)), np.ones(G), np.zeros(G, bool)
        for j in range(G):
            cjj = C[t, j, j]
            flat = mom["mn"][t, j] == mom["mx"][t, j] or cjj <= 0 or D == 1
            dj = cjj
            for k in range(j):
                if not kept[k]:
                    continue
                a = C[t, k, j]
                for q in range(k):
                    a -= Lm[j, q] * Lm[k, q] * dd[q]
                Lm[j, k] = a / dd[k]
                dj -= Lm[j, k] * Lm[j, k] * dd[k]
            if not flat:
                ratio[t, j] = dj / cjj
                kept[j] = dj > tau * cjj
            if kept[j]:
                dd[j] = dj
            else:
                Lm[j, :] = 0.0
        w = np.where(kept, c[t], 0.0)
        for j in range(G):
            for k in range(j):
                w[j] -= Lm[j, k] * w[k]
        w = w / dd
        for j in range(G - 1, -1, -1):
            for i in range(j + 1, G):
                w[j] -= Lm[i, j] * w[i]
        w = np.where(kept, w, 0.0)
        b0 = ybar - float((w * mean[t]).sum())
        ls = max(0.0, syy_D - float((w * c[t]).sum()))
        with np.errstate(over="ignore"):
            if not np.isfinite(np.concatenate([[b0], w]).astype(np.float32)).all():
                continue
        loss[t], coef[t, 0], coef[t, 1:] = ls, b0, w
        kept_all[t] = kept
        if kept.any():
            K = np.flatnonzero(kept)
            s = 1.0 / np.sqrt(np.diagonal(C[t])[K])
            cond[t] = np.linalg.cond(C[t][np.ix_(K, K)] * s[:, None] * s[None, :])
    return dict(loss=loss, coef=coef, kept=kept_all, ratio=ratio, cond=cond)


def fit(Gv, y):
    """moments and the rules in one go: the merged dict"""
    mom = moments(Gv, y)
    return dict(mom, **solve(mom))


def borderline(ratio, lo=2.0 ** -40, hi=2.0 ** -20):
    """(pop,) bool: some d_j / C_jj of the tree lies in [lo, hi]"""
    with np.errstate(invalid="ignore"):
        return ((ratio >= lo) & (ratio <= hi)).any(axis=1)
