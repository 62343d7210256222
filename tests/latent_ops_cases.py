"""Cases, references and error bounds of the latent-Vecchia operator tests, shared by
tests/test_gpu_latent_ops.py (the HIP kernels through the GPB_TestLatentOps* hooks) and
tests/test_latent_ops_reference.py (CPU: every case reaches the dispatch path it is named for, shown from its
neighbour table alone by a numpy restatement of the structure builder's greedy cutting, and float64 numpy
stand-ins of every operation meet the very bounds the kernels are held to).

B is unit lower triangular in Vecchia order: row i holds 1 on the diagonal and Bv[i][r] at column nbr[i][r],
r < k_i = min(i, m). Inputs are float64, references numpy.longdouble. The bounds assume a 64-bit significand
(x87 extended precision: eps = 2^-63); assert_longdouble() checks that and both test files call it.

Bounds, u = 2^-53; none of them tuned to what a kernel gives.
  operators  row with k terms (entries, the unit term, W.*H), S = |pre_i x_i| + sum |v||pre||x| + |W||H|:
             |y^ - y| <= (k + 4) u |scale| S + (k + 4) 2^-64 S. A sum of k terms in ANY order and with any mix of
             fma and separate roundings has error <= gamma_{k-1} S (Higham, Accuracy and Stability, eq. 3.5 and
             section 4.2: the bound does not depend on the order); the 4 covers the v * pre product, the scale
             and one spare. The second term is the longdouble reference's own error.
  ApplyA     V = B^T (Dinv .* (B H)) + W .* H: the operator bound twice. With S1 = |B||H| (k1 terms) the inner
             block G has |dG| <= (k1 + 4) u Dinv S1 and |G| <= Dinv S1, so
             |dV| <= |B|^T |dG| + (k2 + 4) u (|B|^T Dinv S1 + |W||H|), u -> u + 2^-64 for the reference.
  precond    z = B^-1 diag(1/dw) B^-T r. With B = I + N, |B^-1| <= (I - |N|)^-1 = M(B)^-1, M(B) = 2I - |B|
             (a Neumann series, convergent since every row of |N| sums to <= 0.9). Every method of the plan
             (substitution in any order, merged levels with substituted coefficient products, the explicit
             inverse G = B_00^-1 applied by MFMA products) evaluates z as a sum over dependency paths of
             products of B entries, so the error of an entry is at most (the roundings on the longest path)
             times the sum of the absolute path products, which is e = M^-1 diag(1/dw) M^-T |r|:
             |z^ - z| <= C u e, C = 2 (depth + 1)(m + 3) + 4 ld0 (depth: longest dependency chain, m + 3
             roundings per row and solve: m products-and-adds, the input, the division, one spare; ld0: the
             dense head's padded order, the length of its MFMA dot products, twice per product, two
             products). Xt = B^-T r is held to C / 2 and e_t = M^-T |r|. Plain float64 substitution lands at
             0.7 to 6 u e and an explicit float64 inverse at 1.5 to 17 u e on these cases
             (tests/test_latent_ops_reference.py prints them), C being 1e4 to 9e4: the bound is loose against rounding and still 10^8 below a missing or misplaced entry.
"""
import ctypes
import functools

import numpy as np

from gpboost_amd import synthetic

U = 2.0 ** -53
UREF = 2.0 ** -64
LD = np.longdouble
K_LONG_ROW, K_SEG_ENTRIES, K_SEG_ROWS, K_TILE_ROWS, K_TILE_UNION = 64, 512, 127, 64, 176

STATS = ("nnz", "max_list", "min_list", "nlong", "nseg", "seg_by_entries", "seg_by_rows", "seg_overlong", "seg_pad",
         "tile_b", "fb_b", "umax_b", "tile_bt", "fb_bt", "umax_bt", "K0", "K", "ld0", "tail_bt", "tail_low",
         "seg_passes", "launches")
OPT_KEYS = ("relabel", "dense_rows", "head_rows", "tail_merge", "seg_form", "tail_order", "tail_form", "tail_w",
            "no_graph")
OP_B, OP_BT, OP_A, OP_PRECOND = 0, 1, 2, 3
# LatentBForm / LatentBtForm (gpboost_amd/csrc/latent_test.h)
B_FORMS = {"ell": 1, "groups": 2, "old": 3, "wave16": 4, "wave32": 5, "ch0": 6, "ch16": 7, "ch0p": 8, "ch16p": 9,
           "tiled": 10}
BT_FORMS = {"paired": 1, "e2": 2, "e4": 3, "s2": 4, "shfl": 5, "e1": 6, "groups": 7, "old": 8, "wave16": 9,
            "wave32": 10, "ch0": 11, "ch16": 12, "ch0p": 13, "ch16p": 14, "tiled": 15}
T_ALL = (1, 2, 3, 17, 51, 64, 65, 100)
T_LARGE = (1, 3, 51, 65)
HUB_COUNTS = (63, 64, 65, 127, 128, 129, 175, 176, 177, 511, 512, 513)
KNN_M = (1, 5, 16, 17, 30, 32, 33, 64, 65)


def assert_longdouble():
    fi = np.finfo(LD)
    assert fi.nmant == 63 and fi.eps == 2.0 ** -63, f"numpy.longdouble has a {fi.nmant + 1}-bit significand, not 64"


def max_ratio(err, bound):
    """largest err / bound over the entries (0 / 0 counts as 0, err > 0 = bound as inf, NaN as inf)"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0., 0., err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r))


# ------------------------------------------------------------------------------------------------ structures
def _banded(n, m):
    nbr = np.zeros((n, m), dtype=np.int32)
    for i in range(1, n):
        k = min(i, m)
        nbr[i, :k] = i - 1 - np.arange(k)
    return nbr


def _star(n, m):
    """row i takes row 0 and its m - 1 predecessors: column 0's list has n - 1 entries"""
    nbr = _banded(n, m)
    for i in range(m + 1, n):
        nbr[i, m - 1] = 0
    return nbr


def _hubs(m=8, gap=200):
    """a chain (every column one entry) whose columns 10 + gap k receive HUB_COUNTS[k] entries in all: the
    rows c + 2 .. c + T of hub column c take it as a further neighbour (at most three hubs overlap)"""
    cols = [10 + gap * k for k in range(len(HUB_COUNTS))]
    n = cols[-1] + HUB_COUNTS[-1] + 30
    nbr = np.zeros((n, m), dtype=np.int32)
    fill = np.zeros(n, dtype=np.int64)
    for i in range(1, n):
        nbr[i, 0] = i - 1
        fill[i] = 1
    for c, T in zip(cols, HUB_COUNTS):
        for i in range(c + 2, c + T + 1):
            nbr[i, fill[i]] = c
            fill[i] += 1
    # rows i < m hold min(i, m) entries by the layout's rule: give the first rows their full lists
    for i in range(1, m):
        nbr[i, :i] = i - 1 - np.arange(i)
    assert cols[0] > m and fill.max() <= m
    # the layout has k_i = min(i, m) entries in every row: fill the unused slots with distinct earlier rows far
    # from every hub column (rows 0 .. m - 1 plus non-hub predecessors)
    hubset = set(cols)
    for i in range(m, n):
        used = set(nbr[i, :fill[i]].tolist())
        j = i - 2
        while fill[i] < m:
            if j not in used and j not in hubset:
                nbr[i, fill[i]] = j
                fill[i] += 1
            j -= 1
    return nbr, cols


CASES = {f"knn-{m}": ("knn", 700, m) for m in KNN_M}
CASES.update({"star": ("star", 1300, 30), "hubs": ("hubs", 0, 8), "chain": ("chain", 400, 1)})
CASES.update({f"tiny-{n}-{m}": ("tiny", n, m) for n in (1, 2, 3, 65) for m in (1, 5, 70)})
LARGE = ("star", "hubs")


def t_set(name):
    return T_LARGE if name in LARGE else T_ALL


@functools.lru_cache(maxsize=None)
def structure(name):
    """(coordinates n x 2, nbr n x m int32) of a case, in Vecchia order"""
    kind, n, m = CASES[name]
    if kind == "knn":
        from oracle import oracle as O
        _, xv, nbr = O.vecchia_setup(synthetic.bench_coords(n), m, 0, True)
        nbr = np.ascontiguousarray(nbr, dtype=np.int32)
        for i in range(min(n, m)):
            nbr[i, i:] = 0
        return np.ascontiguousarray(xv, dtype=np.float64), nbr
    if kind == "hubs":
        nbr, _ = _hubs(m)
    elif kind == "star":
        nbr = _star(n, m)
    else:
        nbr = _banded(n, m)
    X = np.random.default_rng(len(name) + 7 * nbr.shape[0]).random((nbr.shape[0], 2))
    return X, nbr


def kcount(n, m):
    return np.minimum(np.arange(n), m)


def check_structure(nbr):
    n, m = nbr.shape
    for i in range(n):
        k = min(i, m)
        row = nbr[i, :k]
        assert ((row >= 0) & (row < i)).all(), i
        assert len(set(row.tolist())) == k, i


# ---------------------------------------------- restatement of LatentVecchia::BuildStructure (storage = Vecchia order)
def transposed(nbr):
    """(tptr, trow, tslot): column j -> rows ascending"""
    n, m = nbr.shape
    k = kcount(n, m)
    mask = np.arange(m)[None, :] < k[:, None]
    rows, slots = np.nonzero(mask)
    cols = nbr[rows, slots]
    order = np.lexsort((slots, rows, cols))
    order = order[np.argsort(cols[order], kind="stable")]
    tptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(tptr, cols + 1, 1)
    tptr = np.cumsum(tptr)
    return tptr, rows[order].astype(np.int64), (rows[order] * m + slots[order]).astype(np.int64)


def segment_runs(tptr, trow):
    """greedy runs of consecutive rows (<= K_SEG_ENTRIES entries or one longer row, <= K_SEG_ROWS rows), the packed
    word of every entry, and how each closed run was closed"""
    n = len(tptr) - 1
    seg, closed = [0], []
    pk = np.zeros(max(int(tptr[n]), 1), dtype=np.uint64)
    ce = cr = 0
    for j in range(n):
        ln = int(tptr[j + 1] - tptr[j])
        if cr > 0 and (ce + ln > K_SEG_ENTRIES or cr >= K_SEG_ROWS):
            closed.append("rows" if cr >= K_SEG_ROWS else "entries")
            seg.append(j)
            ce = cr = 0
        for e in range(int(tptr[j]), int(tptr[j + 1])):
            pk[e] = int(trow[e]) | (cr << 24) | ((1 << 31) if e + 1 == tptr[j + 1] else 0)
        ce += ln
        cr += 1
    seg.append(n)
    return np.array(seg), pk, closed


def tile_plan(nbr, tptr, trow, trans):
    """(tiles, fallback rows, largest union) of the greedy LDS tile cutting"""
    n, m = nbr.shape
    i = tiles = umax = nfb = 0
    while i < n:
        start, rows, union = i, 0, set()
        while i < n and i - start < K_TILE_ROWS:
            ids = trow[tptr[i]:tptr[i + 1]] if trans else nbr[i, :min(i, m)]
            if len(ids) > K_TILE_UNION:
                nfb += 1
                i += 1
                continue
            new = set(int(x) for x in ids) - union
            if rows > 0 and len(union) + len(new) > K_TILE_UNION:
                break
            union |= new
            rows += 1
            i += 1
        umax = max(umax, len(union))
        tiles += 1
    return tiles, nfb, umax


@functools.lru_cache(maxsize=None)
def expected_stats(name):
    """what GPB_TestLatentOpsInfo must return for the structure part with relabel = 0"""
    _, nbr = structure(name)
    n, m = nbr.shape
    tptr, trow, _ = transposed(nbr)
    ln = np.diff(tptr)
    seg, pk, closed = segment_runs(tptr, trow)
    runlen = tptr[seg[1:]] - tptr[seg[:-1]]
    tb, tbt = tile_plan(nbr, tptr, trow, False), tile_plan(nbr, tptr, trow, True)
    return dict(nnz=int(tptr[n]), max_list=int(ln.max()), min_list=int(ln.min()), nlong=int((ln > K_LONG_ROW).sum()),
                nseg=len(seg) - 1, seg_by_entries=closed.count("entries"), seg_by_rows=closed.count("rows"),
                seg_overlong=int((ln > K_SEG_ENTRIES).sum()), seg_pad=int((runlen & 1).sum()),
                tile_b=tb[0], fb_b=tb[1], umax_b=tb[2], tile_bt=tbt[0], fb_bt=tbt[1], umax_bt=tbt[2],
                _runlen=runlen, _seg=seg, _pk=pk, _tptr=tptr, _trow=trow)


def depth(nbr):
    n, m = nbr.shape
    lvl = np.zeros(n, dtype=np.int64)
    for i in range(1, n):
        lvl[i] = lvl[nbr[i, :min(i, m)]].max() + 1
    return int(lvl.max()) + 1


# ------------------------------------------------------------------------------------------------ values
def _rng(name, salt):
    return np.random.default_rng([sum(map(ord, name)), salt])


def _decades(rng, n):
    return 10.0 ** rng.uniform(-1.5, 1.5, n)


@functools.lru_cache(maxsize=None)
def values(name, kind="rand"):
    """dict Bv, alt (n x m), Dinv, W, dw (n): signed weights with sum |b| <= 0.9 per row, positive vectors over
    three decades. kind 'krig' (knn cases): Bv, Dinv of the exponential covariance's latent Vecchia factor."""
    X, nbr = structure(name)
    n, m = nbr.shape
    rng = _rng(name, 1)
    mask = np.arange(m)[None, :] < kcount(n, m)[:, None]

    def weights():
        b = rng.uniform(-1., 1., (n, m)) * mask
        s = np.abs(b).sum(axis=1, keepdims=True)
        return np.where(s > 0, b / np.where(s > 0, s, 1.) * rng.uniform(0.45, 0.9, (n, 1)), 0.)
    out = dict(Bv=weights(), alt=weights(), Dinv=_decades(rng, n), W=_decades(rng, n))
    if kind == "krig":
        from oracle import oracle as O
        f = O.latent_factor(X, nbr, 0, O.transform_latent(0, [1.0, 0.15]))
        out["Bv"], out["Dinv"] = np.ascontiguousarray(f["B"] * mask), np.ascontiguousarray(f["Dinv"])
    out["dw"] = out["Dinv"] + out["W"]
    for k in ("Bv", "alt"):
        out[k] = np.ascontiguousarray(out[k])
    return out


@functools.lru_cache(maxsize=None)
def block(name, t, salt):
    """standard normal n x t, a distinct value per (row, column)"""
    n = structure(name)[1].shape[0]
    return _rng(name, 100 * salt + 7).standard_normal((n, t))


@functools.lru_cache(maxsize=None)
def vector(name, salt):
    n = structure(name)[1].shape[0]
    return _decades(_rng(name, 1000 + salt), n)


# ------------------------------------------------------------------------------------------------ references
def _entries(nbr):
    n, m = nbr.shape
    k = kcount(n, m)
    for r in range(m):
        rows = np.nonzero(k > r)[0]
        if rows.size:
            yield r, rows, nbr[rows, r]


_TRANSPOSED = {}


def _transposed_of(nbr):
    key = (nbr.shape, nbr.tobytes())
    if key not in _TRANSPOSED:
        if len(_TRANSPOSED) > 64:
            _TRANSPOSED.clear()
        _TRANSPOSED[key] = transposed(nbr)
    return _TRANSPOSED[key]


def ref_b(nbr, V, unit, X, scale, absolute=False):
    """diag(scale)(unit X + V X) in longdouble; absolute: (k, S) of the bound instead (S without the scale)"""
    n, m = nbr.shape
    f = np.abs if absolute else (lambda a: a)
    X, V = f(X.astype(LD)), f(V.astype(LD))
    Y = X.copy() if unit else np.zeros_like(X)
    for r, rows, cols in _entries(nbr):
        Y[rows] += V[rows, r, None] * X[cols]
    if absolute:
        return kcount(n, m) + (1 if unit else 0), Y
    return Y * scale.astype(LD)[:, None] if scale is not None else Y


def ref_bt(nbr, V, unit, X, pre, W, H, absolute=False):
    """unit pre.*X + V^T (pre.*X) + W.*H in longdouble; absolute: (k, S) of the bound"""
    n, m = nbr.shape
    f = np.abs if absolute else (lambda a: a)
    X, V = f(X.astype(LD)), f(V.astype(LD))
    PX = X * f(pre.astype(LD))[:, None] if pre is not None else X
    Y = PX.copy() if unit else np.zeros_like(X)
    tptr, trow, tslot = _transposed_of(nbr)
    cnt = np.diff(tptr)
    if len(trow):
        terms = V.reshape(-1)[tslot][:, None] * PX[trow]
        full = cnt > 0          # between two non-empty lists' starts lie exactly the first one's entries
        Y[full] += np.add.reduceat(terms, tptr[:-1][full], axis=0)
    if W is not None:
        Y += f(W.astype(LD))[:, None] * f(H.astype(LD))
    if absolute:
        return cnt + (1 if unit else 0) + (1 if W is not None else 0), Y
    return Y


def op_bound(k, S, scale=None):
    kk = (k + 4).astype(np.float64)[:, None]
    sc = np.abs(scale)[:, None] if scale is not None else 1.
    return (kk * U * sc * S + kk * UREF * S).astype(np.float64)


def b_ratio(nbr, V, unit, X, scale, Y):
    ref = ref_b(nbr, V, unit, X, scale)
    k, S = ref_b(nbr, V, unit, X, None, absolute=True)
    return max_ratio(np.abs(Y.astype(LD) - ref), op_bound(k, S, scale))


def bt_ratio(nbr, V, unit, X, pre, W, H, Y):
    ref = ref_bt(nbr, V, unit, X, pre, W, H)
    k, S = ref_bt(nbr, V, unit, X, pre, W, H, absolute=True)
    return max_ratio(np.abs(Y.astype(LD) - ref), op_bound(k, S))


def a_ref_bound(nbr, Bv, D, W, H, carried_in=None):
    """(reference, bound) of B^T (D .* (B H)) + W .* H: the operator bound applied twice. carried_in (nullable):
    an error already in H, carried through |B|^T D |B| + |W|."""
    G = ref_b(nbr, Bv, 1, H, D)
    ref = ref_bt(nbr, Bv, 1, G, None, W, H)
    k1, S1 = ref_b(nbr, Bv, 1, H, None, absolute=True)
    GS = S1 * D.astype(LD)[:, None]
    dG = (k1 + 4).astype(LD)[:, None] * (U + UREF) * GS
    if carried_in is not None:
        dG = dG + ref_b(nbr, Bv, 1, carried_in, None, absolute=True)[1] * D.astype(LD)[:, None]
    _, carried = ref_bt(nbr, Bv, 1, dG, None, None, None, absolute=True)
    k2, S2 = ref_bt(nbr, Bv, 1, GS, None, W, H, absolute=True)
    bound = carried + (k2 + 4).astype(LD)[:, None] * (U + UREF) * S2
    if carried_in is not None and W is not None:
        bound = bound + np.abs(W).astype(LD)[:, None] * carried_in
    return ref, bound.astype(np.float64)


def a_ratio(nbr, vals, H, V):
    """(B^T Dinv B + W) H against the operator bound applied twice"""
    ref, bound = a_ref_bound(nbr, vals["Bv"], vals["Dinv"], vals["W"], H)
    return max_ratio(np.abs(V.astype(LD) - ref), bound)


# cached pieces of the operator references of a case: the GPU tests run every argument combination and every form
# on the same inputs, so the longdouble products are formed once per (values, block) and combined per combination
@functools.lru_cache(maxsize=48)
def _core_b(name, kind, alt, t):
    _, nbr = structure(name)
    V = values(name, kind)["alt" if alt else "Bv"]
    X = block(name, t, 0)
    return ref_b(nbr, V, 0, X, None), ref_b(nbr, V, 0, X, None, absolute=True)[1]


@functools.lru_cache(maxsize=48)
def _core_bt(name, kind, alt, with_pre, t):
    _, nbr = structure(name)
    V = values(name, kind)["alt" if alt else "Bv"]
    X = block(name, t, 0)
    pre = vector(name, 1) if with_pre else None
    k, S = ref_bt(nbr, V, 0, X, pre, None, None, absolute=True)
    return ref_bt(nbr, V, 0, X, pre, None, None), S, k


def case_inputs(name, t):
    """X, H (n x t), scale, pre, W (n) of a case's operator tests"""
    return block(name, t, 0), block(name, t, 1), vector(name, 0), vector(name, 1), vector(name, 2)


def case_b_ratio(name, kind, alt, unit, with_scale, t, Y):
    X, _, scale, _, _ = case_inputs(name, t)
    core, acore = _core_b(name, kind, alt, t)
    n, m = structure(name)[1].shape
    ref, S = (core + X.astype(LD), acore + np.abs(X).astype(LD)) if unit else (core, acore)
    if with_scale:
        ref = ref * scale.astype(LD)[:, None]
    return max_ratio(np.abs(Y.astype(LD) - ref), op_bound(kcount(n, m) + (1 if unit else 0), S,
                                                          scale if with_scale else None))


def case_bt_ratio(name, kind, alt, unit, with_pre, with_wh, t, Y):
    X, H, _, pre, W = case_inputs(name, t)
    core, acore, cnt = _core_bt(name, kind, alt, with_pre, t)
    ref, S, k = core, acore, cnt
    if unit:
        PX = X.astype(LD) * (pre.astype(LD)[:, None] if with_pre else 1)
        ref, S, k = ref + PX, S + np.abs(PX), k + 1
    if with_wh:
        WH = W.astype(LD)[:, None] * H.astype(LD)
        ref, S, k = ref + WH, S + np.abs(WH), k + 1
    return max_ratio(np.abs(Y.astype(LD) - ref), op_bound(k, S))


@functools.lru_cache(maxsize=16)
def case_a_ref_bound(name, kind, t):
    v = values(name, kind)
    return a_ref_bound(structure(name)[1], v["Bv"], v["Dinv"], v["W"], block(name, t, 1))


@functools.lru_cache(maxsize=16)
def case_precond_ref(name, kind, t):
    return precond_ref(structure(name)[1], values(name, kind), block(name, t, 2))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def solve_lower(nbr, N, Y):
    """x with (I + N) x = Y, row by row, in Y's dtype"""
    n, m = nbr.shape
    X = Y.copy()
    for i in range(1, n):
        k = min(i, m)
        X[i] -= (N[i, :k, None] * X[nbr[i, :k]]).sum(axis=0)
    return X


def solve_upper(nbr, N, Y):
    """x with (I + N)^T x = Y, last row first"""
    n, m = nbr.shape
    X = Y.copy()
    for i in range(n - 1, 0, -1):
        k = min(i, m)
        X[nbr[i, :k]] -= N[i, :k, None] * X[i]
    return X


def precond_ref(nbr, vals, R):
    """(z, xt, e, e_t) in longdouble: z = B^-1 diag(1/dw) B^-T R, xt = B^-T R and the bounds' e, e_t"""
    Bv, dw = vals["Bv"].astype(LD), vals["dw"].astype(LD)[:, None]
    xt = solve_upper(nbr, Bv, R.astype(LD))
    z = solve_lower(nbr, Bv, xt / dw)
    et = solve_upper(nbr, -np.abs(Bv), np.abs(R).astype(LD))
    e = solve_lower(nbr, -np.abs(Bv), et / dw)
    return z, xt, e, et


def precond_c(nbr, ld0):
    return 2 * (depth(nbr) + 1) * (nbr.shape[1] + 3) + 4 * ld0


# ------------------------------------------------------------------------------------ the library's test hooks
def _lib():
    c = ctypes
    from gpboost_amd import basic
    lib = basic.lib()
    if not getattr(lib, "_latent_ops_typed", False):
        D, I, L, V = c.POINTER(c.c_double), c.c_int, c.c_int64, c.c_void_p
        PI, PL = c.POINTER(c.c_int32), c.POINTER(c.c_int64)
        lib.GPB_TestLatentOpsCreate.argtypes = [I, I, PI, L, I, D, L, PL, c.POINTER(V)]
        lib.GPB_TestLatentOpsFree.argtypes = [V]
        lib.GPB_TestLatentOpsSetValues.argtypes = [V, D, L, D, D, D, L, D, L]
        lib.GPB_TestLatentOpsInfo.argtypes = [V, PL, L, PI, L]
        lib.GPB_TestLatentOpsApply.argtypes = [V, I, I, I, I, I, D, D, D, D, L, D, D, D, L, c.POINTER(I)]
        lib.GPB_TestLatentOpsVector.argtypes = [I, I, I, I, I, I, c.c_double, c.c_double, c.POINTER(D), L, D, D, PI, L,
                                                D, D, D, L, c.POINTER(I)]
        lib.GPB_TestLatentOpsPcg.argtypes = [V, I, I, c.c_double, I, I, D, D, L, c.POINTER(I), c.POINTER(I)]
        lib.LGBM_GetLastError.restype = c.c_char_p
        lib._latent_ops_typed = True
    return lib


def _dp(a):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a, ty=ctypes.c_int32):
    if a is None:
        return None
    assert a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.POINTER(ty))


def opts_array(opt):
    assert set(opt) <= set(OPT_KEYS), opt
    return np.array([opt.get(k, -1) for k in OPT_KEYS], dtype=np.int64)


def last_error():
    return _lib().LGBM_GetLastError().decode("utf-8")


class HookError(RuntimeError):
    pass


def _check(ret):
    if ret != 0:
        msg = last_error()
        if "HIP error" in msg:          # the device context is gone: nothing more may run on it
            import pytest
            pytest.exit(f"HIP error, session ended: {msg}", returncode=3)
        raise HookError(msg)


VEC_OPS = {"coldots": 0, "cg_update": 1, "h_update": 2, "alpha": 3, "beta": 4, "axpby": 5, "cap_mode": 6, "pack": 7}
VEC_SMALL = {0: lambda np_, t: np_ * t, 1: lambda np_, t: t, 3: lambda np_, t: 2 * t, 4: lambda np_, t: 3 * t}
VEC_N, VEC_T = (1, 255, 257, 2500), (1, 3, 51, 64, 65, 130)


def vector_raw(op, n, t, blocks=(), np_=1, ia=0, ib=0, alpha=0., beta=0., sv0=None, sv1=None, act=None,
               block_len=None, small_len=None, small_out_len=None):
    """GPB_TestLatentOpsVector: returns (return code, out0, out1, small_out, guard flag)"""
    D = ctypes.POINTER(ctypes.c_double)
    arr = (D * 6)(*([_dp(b) for b in blocks] + [None] * (6 - len(blocks))))
    out0, out1 = np.full((n, t), 7.25), np.full((n, t), 7.25)
    ns = VEC_SMALL.get(op, lambda a, b: 0)(np_, t)
    small = np.full(max(ns, 1), 7.25)
    g = ctypes.c_int(-1)
    ret = _lib().GPB_TestLatentOpsVector(op, n, t, np_, ia, ib, alpha, beta, arr, n * t if block_len is None else block_len,
                                         _dp(sv0), _dp(sv1), _ip(act), t if small_len is None else small_len,
                                         _dp(out0), _dp(out1), _dp(small) if ns else None,
                                         ns if small_out_len is None else small_out_len, ctypes.byref(g))
    return ret, out0, out1, small[:ns], g.value


def vec_op(op, n, t, blocks=(), **kw):
    ret, out0, out1, small, g = vector_raw(VEC_OPS[op], n, t, blocks, **kw)
    _check(ret)
    assert g == 0, f"{op}: a guard word changed (n {n}, t {t})"
    return out0, out1, small


def dots_bound(A, B):
    """(reference, bound) of the column sums of A .* B: (n + 2) u sum |a b|, any order, plus the reference's own"""
    P = A.astype(LD) * B.astype(LD)
    return P.sum(axis=0), ((A.shape[0] + 2) * (U + UREF) * np.abs(P).sum(axis=0)).astype(np.float64)


class LatentOps:
    """A GPB_TestLatentOps* handle of one case with its values set"""

    def __init__(self, name, opt=None, kind="rand", set_values=True):
        self.name = name
        self.X, self.nbr = structure(name)
        self.n, self.m = self.nbr.shape
        self.vals = values(name, kind)
        self.h = ctypes.c_void_p()
        o = opts_array(opt or {})
        _check(_lib().GPB_TestLatentOpsCreate(self.n, self.m, _ip(self.nbr), self.nbr.size, self.X.shape[1],
                                              _dp(self.X), self.X.size, _ip(o, ctypes.c_int64), ctypes.byref(self.h)))
        if set_values:
            v = self.vals
            _check(_lib().GPB_TestLatentOpsSetValues(self.h, _dp(v["Bv"]), v["Bv"].size, _dp(v["Dinv"]), _dp(v["W"]),
                                                     _dp(v["dw"]), self.n, _dp(v["alt"]), v["alt"].size))

    def close(self):
        if self.h:
            _lib().GPB_TestLatentOpsFree(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: the library is going away with the process
            pass

    def info(self):
        st = np.zeros(len(STATS), dtype=np.int64)
        vo = np.zeros(self.n, dtype=np.int32)
        _check(_lib().GPB_TestLatentOpsInfo(self.h, _ip(st, ctypes.c_int64), st.size, _ip(vo), vo.size))
        return dict(zip(STATS, (int(x) for x in st))), vo

    def apply_raw(self, op, form, t, unit, alt, X, pre=None, scale=None, W=None, H=None, vec_len=None, block_len=None):
        """returns (return code, Y, Y2, guard flag)"""
        Y, Y2 = np.full((self.n, t), 7.25), np.full((self.n, t), 7.25)
        g = ctypes.c_int(-1)
        ret = _lib().GPB_TestLatentOpsApply(self.h, op, form, t, int(unit), int(alt), _dp(X), _dp(pre), _dp(scale),
                                            _dp(W), self.n if vec_len is None else vec_len, _dp(H), _dp(Y), _dp(Y2),
                                            self.n * t if block_len is None else block_len, ctypes.byref(g))
        return ret, Y, Y2, g.value

    def pcg(self, t, n_single, delta, pmax_single, pmax_block, RHS, block_len=None):
        """returns (return code, U, (its_single, its_block), (nan, zero_rhs))"""
        Uo = np.full((self.n, t), 7.25)
        its, flags = (ctypes.c_int * 2)(-1, -1), (ctypes.c_int * 2)(-1, -1)
        ret = _lib().GPB_TestLatentOpsPcg(self.h, t, n_single, delta, pmax_single, pmax_block, _dp(RHS), _dp(Uo),
                                          self.n * t if block_len is None else block_len, its, flags)
        return ret, Uo, (its[0], its[1]), (flags[0], flags[1])

    def apply(self, op, form, t, unit, alt, X, **kw):
        """Y (and Y2 for the preconditioner); asserts the guards are untouched and every payload entry was written"""
        ret, Y, Y2, g = self.apply_raw(op, form, t, unit, alt, X, **kw)
        _check(ret)
        assert g == 0, f"{self.name}: a guard word changed (op {op}, form {form}, t {t})"
        assert not np.isnan(Y).any(), f"{self.name}: NaN left in the output (op {op}, form {form}, t {t})"
        if op == OP_PRECOND:
            assert not np.isnan(Y2).any(), f"{self.name}: NaN left in Xt (t {t})"
            return Y, Y2
        return Y
