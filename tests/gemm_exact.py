"""Shared by tests/test_gemm_pair_gpu.py, tests/test_kernels_gpu.py and tests/test_gemm_exact_cpu.py: the exact-integer method
for the f32 GEMMs (csrc/gemm.hip), the case tables, and a Python restatement of the host planners that decide which kernel
instantiation a shape takes.

The method.  With every operand drawn from {-1, 0, 1} as float32, every product and every partial sum of a GEMM, of its
BatchNorm column sums (sum C, sum C^2) and of a split weight gradient is an integer; as long as sum |terms| stays below 2^24
every partial sum is a float32 value whatever the order, the tiling or the split.  The device must then give the float64
reference bit for bit: one dropped, duplicated or misplaced row changes an integer.  `premise_*` assert the 2^24 conditions from
the float64 reference (a condition of the test, not a tolerance).  Ternary values survive any reduced-precision path, so the
random-float bars of the callers stay next to the exact runs.

The planners (nn_plan / tn_plan below restate nn_plan / tn_plan_search of gemm.hip) are not visible from outside the library;
tests/test_gemm_exact_cpu.py checks the restatement against kws_gemm_nn_stats_rows / kws_gemm_tn_workspace_floats on every
case, and the GPU tests against the S the launches return, so the labels of the tables cannot drift silently."""
import numpy as np

NXCD = 8
WS_MAX_N = 1024          # KWS_WS_MAX_N
TN_MAX_S = 256           # KWS_TN_MAX_S
LIMIT = float(2 ** 24)


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# the planners, restated
# ---------------------------------------------------------------------------------------------------------------------------
def nn_plan(M, K, N, gather=False):
    """C[M, N] = A[M, K] W[K, N]: dict(ws, bn, kb, wgs, m_tiles, rows); rows = statistics rows of kws_gemm_nn_f32"""
    m_tiles = ceil_div(M, 128)
    bn = 128 if N % 128 == 0 else 64
    if bn == 128 and not gather and K % 64 == 0 and K >= 128:
        t128 = m_tiles * (N // 128)

        def rounds(t):
            e = t % 256
            return float(t // 256) + (0.0 if e == 0 else (0.55 if 2 * e <= 256 else 1.0))
        if 0.55 * rounds(2 * t128) < rounds(t128):
            bn = 64
    kb = 64 if (bn == 64 and K % 64 == 0 and K >= 128) else 32
    slots = ceil_div(m_tiles, NXCD) * ceil_div(N, bn)
    ws = (not gather) and K % kb == 0 and K >= 2 * kb and N % bn == 0 and N <= WS_MAX_N
    wgs = min(slots, 32) * NXCD
    return dict(ws=ws, bn=bn, kb=kb, wgs=wgs, m_tiles=m_tiles, rows=wgs if ws else m_tiles)


def nn_form(M, K, N):
    """the kernel kws_gemm_nn_f32 runs: 'wide' (128-wide tiles, 32-deep slabs), '64/64', '64/32' or 'persistent'"""
    pl = nn_plan(M, K, N)
    if not pl["ws"]:
        return "persistent"
    return "wide" if pl["bn"] == 128 else "64/%d" % pl["kb"]


def nn_edges(M, K, N):
    """the corners of the wave-specialised kernel's tile walk that (M, K, N) reaches (nn_ws_body: an XCD's workgroups walk its
    tiles in rounds; a last round that fits twice is walked in 64-row half tiles)"""
    pl = nn_plan(M, K, N)
    out = set()
    if not pl["ws"]:
        return out
    n_tiles, wpx, m_tiles = N // pl["bn"], pl["wgs"] // NXCD, pl["m_tiles"]
    last_rows = M - (m_tiles - 1) * 128
    for x in range(NXCD):
        panels = (m_tiles - x + NXCD - 1) // NXCD
        local = panels * n_tiles
        full = local // wpx
        e = local - full * wpx
        halves = e > 0 and 2 * e <= wpx
        if local == 0:
            out.add("idle_xcd")
        if full >= 2 or (full == 1 and e > 0):
            out.add("several_rounds")
        if halves:
            out.add("halves_after_full_round" if full >= 1 else "halves_only")
            if x == (m_tiles - 1) % NXCD and (panels - 1) * n_tiles >= full * wpx:     # the last row tile is a half tile
                if last_rows < 64:
                    out.add("half_last_lt64")
                elif last_rows == 64:
                    out.add("half_last_eq64")
                elif last_rows < 128:
                    out.add("half_last_65_127")
        elif x == (m_tiles - 1) % NXCD and local > 0 and last_rows < 128:
            out.add("full_last_ragged")
    return out


def tn_ws_eligible(K, N):
    return K % 64 == 0 and N % 64 == 0


def _tn_cost(M, K, N, tiles, U, chunk):
    S = ceil_div(M, chunk)
    stages = ceil_div(chunk, 32 * U)
    t_stage = 4370 if U == 1 else (4870 if U == 2 else 4550)
    worst = 0
    for x in range(NXCD):
        cnt = (S - x + NXCD - 1) // NXCD if x < S else 0
        per_cu = ceil_div(tiles * cnt, 32)
        worst = max(worst, per_cu * (stages * t_stage + 4500))
    return worst + int(float(S) * K * N * 4.0 * 0.8e-3) + 6000, S


def tn_plan(M, K, N, ws):
    """dW[K, N] = A[M, K]^T G[M, N] in S splits of `chunk` rows: dict(bko, bno, S, chunk, stage); ws = the wave-specialised
    kernel (tile width per dimension), otherwise the 4-wave kernel (square tiles)"""
    if ws:
        bko, bno = (128 if K % 128 == 0 else 64), (128 if N % 128 == 0 else 64)
    else:
        bko = bno = 128 if (K % 128 == 0 and N % 128 == 0) else 64
    tiles = ceil_div(K, bko) * ceil_div(N, bno)
    if not ws:
        S = min(ceil_div(768, tiles), 256, max(M // 256, 1))
        chunk = max(ceil_div(ceil_div(M, S), 128) * 128, 128)
        return dict(bko=bko, bno=bno, S=ceil_div(M, chunk), chunk=chunk, stage=128)
    U = 4 // ((bko // 64) * (bno // 64))
    g = 32 * U
    s_lo = max(1, ceil_div(M, TN_MAX_S * g))
    max_chunk = ((1 << 31) - 1) // (4 * max(K, N))
    best, best_chunk = -1, s_lo * g
    for st in range(s_lo, s_lo * 16 + 64):
        if st * g > max_chunk and st > s_lo:
            break
        c, S = _tn_cost(M, K, N, tiles, U, st * g)
        if best < 0 or c < best:
            best, best_chunk = c, st * g
        if S <= 1:
            break
    return dict(bko=bko, bno=bno, S=ceil_div(M, best_chunk), chunk=best_chunk, stage=g)


def tn_workspace_floats(M, K, N):
    return max(tn_plan(M, K, N, tn_ws_eligible(K, N))["S"], tn_plan(M, K, N, False)["S"]) * K * N


def tn_edges(M, K, N):
    pl = tn_plan(M, K, N, True)
    out = {"S=1" if pl["S"] == 1 else "S>1"}
    if M < pl["stage"]:
        out.add("below_one_stage")
    if pl["S"] > 1 and M % pl["chunk"]:
        out.add("ragged_last_split")
    if M % pl["stage"]:
        out.add("ragged_last_stage")
    return out


def pair_form(M, cin, cout):
    """kws_gemm_dgrad_wgrad_f32 (dZ[M, cin] = dY[M, cout] WT[cout, cin]; slabs of dW[cin, cout] = Z^T dY): None when it refuses
    the shape, else (BN, KB, BKO, BNO) of the gemm_dgrad_wgrad_kernel instantiation it launches"""
    np_ = nn_plan(M, cout, cin)
    if not np_["ws"] or not tn_ws_eligible(cin, cout):
        return None
    return (np_["bn"], np_["kb"], 128 if cin % 128 == 0 else 64, 128 if cout % 128 == 0 else 64)


# the instantiations launch_pair can reach: BN = 128 needs cin % 128 == 0, which makes BKO = 128; KB = 32 beside
# BN = 64 needs cout = 64 (BNO = 64) and cin % 128 != 0 (BKO = 64)
PAIR_REACHABLE = [(128, 32, 128, 128), (128, 32, 128, 64), (64, 64, 128, 128), (64, 64, 128, 64), (64, 64, 64, 128),
                  (64, 64, 64, 64), (64, 32, 64, 64)]
PAIR_UNREACHABLE = [(128, 32, 64, 128), (128, 32, 64, 64), (64, 32, 128, 128), (64, 32, 128, 64), (64, 32, 64, 128)]


# ---------------------------------------------------------------------------------------------------------------------------
# inputs, references, comparisons
# ---------------------------------------------------------------------------------------------------------------------------
def ternary(rng, *shape):
    return rng.randint(-1, 2, size=shape).astype(np.float32)


def premise_columns(C64):
    """per column of the float64 product: sum |c| and sum c^2 below 2^24 (then so is every partial sum, in any order)"""
    assert np.array_equal(C64, np.rint(C64))
    assert np.abs(C64).sum(axis=0).max() < LIMIT and (C64 ** 2).sum(axis=0).max() < LIMIT, \
        "shape too large for the exact method: a column sum reaches 2^24"


def premise_tn(A, G):
    """sum over m of |a g| below 2^24 for every element of A^T G"""
    assert (np.abs(A).astype(np.float64).T @ np.abs(G).astype(np.float64)).max() < LIMIT, \
        "shape too large for the exact method: a weight-gradient sum reaches 2^24"


def same_bits(got, ref64):
    """got (float32, from the device) equals the float64 reference exactly (and the reference is a float32 value)"""
    got = np.asarray(got)
    ref64 = np.asarray(ref64, dtype=np.float64)
    return got.shape == ref64.shape and got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref64)


def assert_exact(got, ref64, what):
    if not same_bits(got, ref64):
        g, r = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
        assert g.shape == r.shape, "%s: shape %s, reference %s" % (what, g.shape, r.shape)
        bad = np.argwhere(g != r)
        raise AssertionError("%s differs from the float64 reference in %d of %d elements; first at %s: %r, reference %r" % (
            what, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], r[tuple(bad[0])]))


def nn_inputs(M, K, N):
    """ternary A[M, K], W[K, N]"""
    rng = np.random.RandomState(M + K + N)
    return ternary(rng, M, K), ternary(rng, K, N)


def tn_inputs(M, K, N):
    """ternary A[M, K], G[M, N]"""
    rng = np.random.RandomState(M)
    return ternary(rng, M, K), ternary(rng, M, N)


def pair_inputs(M, cin, cout, exact):
    """dY[M, cout], WT[cout, cin], Z[M, cin]: ternary (exact) or random normal floats"""
    rng = np.random.RandomState(M + 3 * cin + 7 * cout)
    if exact:
        return ternary(rng, M, cout), ternary(rng, cout, cin), ternary(rng, M, cin)
    return (rng.randn(M, cout).astype(np.float32), (rng.randn(cout, cin) * 0.1).astype(np.float32),
            rng.randn(M, cin).astype(np.float32))


def gather_inputs(B):
    """ternary clips x[B, 16000], conv1 weights W[3, 40, 128] and a gradient G[B 399, 128] of the headline net's frame + conv1 gather"""
    rng = np.random.RandomState(5 + B)
    return ternary(rng, B, 16000), ternary(rng, 3, 40, 128), ternary(rng, B * 399, 128)


def f64(a):
    return np.asarray(a, dtype=np.float64)


# the headline net's first convolution as a gather (model.py: overlapping_time_slice_stack(40, 20, SAME) + Conv1D(128, 3, strides=2))
GATHER_DESC = dict(L_out=399, cin=40, taps=3, stride_t=40, stride_j=20, base_off=-10, x_len=16000, x_batch_stride=16000)


def gather_ref(x, W):
    """float64 C[B 399, 128] of the gathered GEMM and its unfolded operand cols[B 399, 120]"""
    from oracle import layers as OL
    y, cols = OL.conv1d_fwd(OL.frame_same(f64(x), 40, 20), f64(W), stride=2)
    return y.reshape(-1, W.shape[2]), cols


def tn_without_row(ref64, A, G, r):
    """the weight gradient a kernel that DROPS row r of the M dimension would give"""
    return ref64 - np.outer(f64(A[r]), f64(G[r]))


def tn_with_row_twice(ref64, A, G, r):
    return ref64 + np.outer(f64(A[r]), f64(G[r]))


def tn_controls_row(A, G):
    """the last row whose outer product is non-zero"""
    nz = np.nonzero(np.abs(A).sum(axis=1) * np.abs(G).sum(axis=1))[0]
    assert nz.size
    return int(nz[-1])


def stats_ref(C64):
    """[2, N]: the BatchNorm column sums of C"""
    return np.stack([C64.sum(axis=0), (C64 ** 2).sum(axis=0)])


def stats_without_row(C64, r):
    """the sums an epilogue that DROPS row r would give (host-side sensitivity control)"""
    return stats_ref(C64) - np.stack([C64[r], C64[r] ** 2])


def stats_with_row_twice(C64, r):
    """the sums an epilogue that counts row r TWICE would give"""
    return stats_ref(C64) + np.stack([C64[r], C64[r] ** 2])


def controls_row(C64):
    """a row for the controls: the last one whose values are non-zero (a ragged tile's rows come last)"""
    nz = np.nonzero(np.abs(C64).sum(axis=1))[0]
    assert nz.size, "the product is all zeros"
    return int(nz[-1])


# ---------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------
# kws_gemm_dgrad_wgrad_f32 (M, cin, cout) -> the instantiation <BN, KB, BKO, BNO> and the corners it is there for.  NN side:
# K = cout, N = cin; BN = 128 survives the planner's round pricing only for cout = 64 or m_tiles cin / 128 in 193 .. 256.
PAIR_CASES = [
    # (M, cin, cout, <BN, KB, BKO, BNO>, corners of the NN walk that must be among nn_edges(M, cout, cin))
    # 9 row tiles, 64-wide: seven XCDs hold one row tile each and walk its two column tiles as four halves; last tile 76 rows
    (1100, 128, 128, (64, 64, 128, 128), {"halves_only", "full_last_ragged"}),
    (1180, 128, 192, (64, 64, 128, 64), {"halves_only", "full_last_ragged"}),        # 10 row tiles, the last of 28 rows
    # 40 row tiles x 16 column tiles: 80 items on an XCD's 32 workgroups = 2 rounds + 16 -> halves; the last tile (100 rows) is one
    (5092, 1024, 128, (64, 64, 128, 128), {"halves_after_full_round", "half_last_65_127"}),
    # cout = 64 keeps BN = 128 (K < 128): 40 x 8 items = 1 round + 8 -> halves; last tile 58 rows: its second half is empty
    (5050, 1024, 64, (128, 32, 128, 64), {"halves_after_full_round", "half_last_lt64"}),
    (4096, 1024, 128, (128, 32, 128, 128), set()),                    # m_tiles cin / 128 = 256: BN = 128 survives, one exact round
    (3100, 1024, 192, (128, 32, 128, 64), {"full_last_ragged"}),      # 200 in 193 .. 256; last tile 28 rows in a full-tile walk
    (700, 192, 128, (64, 64, 64, 128), {"idle_xcd", "full_last_ragged"}),            # 6 row tiles: two XCDs idle; last 60 rows
    (100, 64, 128, (64, 64, 64, 128), {"idle_xcd"}),                  # one row tile; two ragged TN splits of 64 + 36 rows
    (1500, 192, 192, (64, 64, 64, 64), {"halves_only"}),              # C3's 192-wide layers; 12 row tiles
    (3000, 64, 64, (64, 32, 64, 64), {"full_last_ragged"}),           # C3's first block (K = 64: 32-deep slabs)
    (1090, 320, 64, (64, 32, 64, 64), {"halves_only", "full_last_ragged"}),          # 9 row tiles x 5 column tiles; last 66 rows
    (100, 64, 64, (64, 32, 64, 64), {"idle_xcd"}),                    # below one 128-row TN stage: S = 1
    (1, 128, 128, (64, 64, 128, 128), {"idle_xcd"}),                  # one row: below one TN stage, S = 1
    (2048, 512, 512, (64, 64, 128, 128), set()),                      # C3's widest layer at a small batch
    (2600, 384, 256, (64, 64, 128, 128), {"full_last_ragged"}),       # C3 widths
    (3333, 256, 320, (64, 64, 128, 64), {"full_last_ragged"}),        # C3 widths, odd M
]
# corners the table as a whole must reach: NN walk (nn_edges) and TN split (tn_edges)
PAIR_NN_CORNERS = {"halves_only", "halves_after_full_round", "half_last_lt64", "half_last_65_127", "full_last_ragged", "idle_xcd",
                   "several_rounds"}
PAIR_TN_CORNERS = {"S=1", "S>1", "below_one_stage", "ragged_last_split", "ragged_last_stage"}
PAIR_REFUSED = [(1000, 120, 128), (1000, 128, 96), (1000, 100, 64)]   # cin % 64, cout % 64: returns 1, nothing written

# kws_gemm_nn_f32 (M, K, N): the list of test_gemm_nn_and_stats ...
NN_CASES = [(1000, 128, 128), (777, 192, 320), (129, 512, 512), (5, 120, 64), (2560, 384, 192), (128, 64, 64), (1, 64, 128),
            (127, 96, 192), (40000, 64, 128), (33000, 128, 256), (4100, 256, 1024), (300, 48, 128), (70000, 160, 64),
            (33692, 128, 128), (33856, 192, 384), (34000, 128, 192)]
# ... + the small half-tile shapes of the pair table as forward GEMMs (K = cout, N = cin); (5, 120, 64) and (300, 48, 128) above
# are the two fallbacks to the persistent kernel
NN_EXACT_CASES = NN_CASES + [(1100, 128, 128), (1180, 192, 128), (5092, 128, 1024), (5050, 64, 1024), (1500, 192, 192),
                             (1090, 64, 320)]

# kws_gemm_tn_f32 (M, K, N): the list of test_gemm_tn
TN_CASES = [(4000, 128, 128), (999, 192, 256), (130, 320, 320), (9216, 512, 512), (100, 64, 64), (5000, 64, 128), (70000, 128, 64),
            (33, 256, 192), (2000, 120, 128), (100000, 192, 192), (777, 64, 100), (1, 128, 128)]

# kws_gemm_gather_f32 with statistics: clips of the headline frame + conv1 gather (399 rows each, K = 120, N = 128); 3 and 11
# clips end in a ragged tile (45 and 37 rows), 165 clips are 515 row tiles: more than one round of the persistent kernel's grid
GATHER_B = [3, 11, 165]

# kws_bn_stats_finalize: one shape per NN form, N = 64 and N = 1024, M not a multiple of 64
BN_CASES = [(3000, 128, 192, "64/64"), (1001, 64, 1024, "wide"), (4100, 256, 1024, "64/64"), (3001, 64, 64, "64/32"),
            (777, 48, 128, "persistent")]
