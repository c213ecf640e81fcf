"""Cases, exact inputs, float64 references and the host-side planner mirror of the grouped depthwise Conv1D kernels
(csrc/gdwconv.hip: kws_gdwconv_*).  A plain module: no fixtures.  Shared by tests/test_gdwconv_kernels_gpu.py (device, bit for bit)
and tests/test_top_down_cpu.py (planner and domain, no device).

Inputs are small integers, or dyadic fractions where a table is applied (scales are powers of two, so scale * x + shift is an
integer or a short dyadic): every product and every partial sum is exact in float32 whatever the order, so the device must equal
the float64 reference bit for bit.  The references are written as slice sums over the tensors, not as the kernels index them."""
import numpy as np

ACT_NONE, ACT_BN, ACT_BIAS = 0, 1, 2
DESC_MEMBERS = ["B", "L", "C", "Lout", "k", "stride", "g", "gs", "x0", "x_step", "act", "bn_group", "w_group_stride"]
SLACK = 1000.0     # what lies between the groups' kernels, and in the table rows no kernel may read


def _case(B, L, C, g, gs, k, s, x_step=None, x0=0, act=ACT_NONE, bn_group=0, w_gap=0, seed=0):
    c = dict(B=B, L=L, C=C, g=g, gs=gs, k=k, stride=s, x0=x0, x_step=gs if x_step is None else x_step, act=act, bn_group=bn_group,
             Lout=(L - k) // s + 1, seed=seed)
    c["w_group_stride"] = k * gs + w_gap if w_gap else 0
    return c


CASES = {
    # dA zeros at row 9 (no window reaches it) and at channels 12 .. 19 (no group reads them)
    "sliced_unread": _case(3, 10, 20, 3, 4, 3, 2, seed=1),
    # every group reads all 12 channels: dA sums both groups
    "shared": _case(2, 7, 12, 2, 12, 3, 1, x_step=0, seed=2),
    # tables of 6 channels under vectors of 4: channels 4 .. 7 straddle tables 0 and 1; pre-activations on 0 and 6
    "table_straddle": _case(2, 9, 12, 3, 4, 3, 1, act=ACT_BN, bn_group=6, seed=3),
    "bias": _case(2, 8, 8, 2, 4, 3, 2, act=ACT_BIAS, seed=4),
    # the windows start at channel 4; the kernels lie 3 * 4 + 9 floats apart (odd: group 1's is not 16-byte aligned)
    "offset_strided": _case(2, 9, 16, 2, 4, 3, 1, x0=4, w_gap=9, seed=5),
    "k5_s3": _case(2, 17, 8, 2, 4, 5, 3, seed=6),
    # windows [0, 8) and [4, 12) overlap: channels 4 .. 7 take both groups' gradients
    "overlap": _case(2, 8, 12, 2, 8, 3, 1, x_step=4, seed=7),
    # 703 output rows: several partial rows, and more than one row per row lane
    "many_rows": _case(37, 21, 24, 2, 12, 3, 1, seed=8),
    # the model's third block at its real widths: 300 of 420 channels through tables of 210, 75 vectors = two column tiles, the
    # kernels as far apart as the model's pointwise kernel and BatchNorm pair put them
    "model_block3": _case(2, 46, 420, 3, 100, 3, 2, act=ACT_BN, bn_group=210, w_gap=100 * 120 + 2 * 120, seed=9),
    # the model's second block: both groups read all 420 channels through tables of 140
    "model_block2": _case(2, 48, 420, 2, 420, 3, 1, x_step=0, act=ACT_BN, bn_group=140, seed=10),
}

# (changes to CASES['sliced_unread'], why the descriptor is outside the domain)
REFUSED = [
    (dict(k=0), "no taps"), (dict(k=8, L=20), "eight taps"), (dict(stride=0), "stride 0"), (dict(stride=5, Lout=2), "stride 5"),
    (dict(g=0), "no groups"), (dict(g=9, C=40), "nine groups"), (dict(gs=6, x_step=6), "gs not a multiple of 4"),
    (dict(gs=0, x_step=0), "empty groups"), (dict(C=22), "C not a multiple of 4"), (dict(x0=2), "x0 not a multiple of 4"),
    (dict(x_step=2), "x_step not a multiple of 4"), (dict(x0=12), "last window past C"), (dict(x_step=12), "windows past C"),
    (dict(x0=-4), "negative x0"), (dict(Lout=5), "windows past L"), (dict(Lout=0), "no output rows"), (dict(B=0), "empty batch"),
    (dict(act=3), "unknown act"), (dict(act=ACT_BN, bn_group=0), "table without bn_group"),
    (dict(act=ACT_BN, bn_group=8), "bn_group does not divide C"), (dict(w_group_stride=11), "w_group_stride below one kernel"),
]


def refused(changes):
    return dict(CASES["sliced_unread"], **changes)


def in_domain(c):
    return (c["B"] > 0 and c["L"] > 0 and c["C"] > 0 and c["Lout"] > 0 and c["gs"] > 0 and 1 <= c["k"] <= 7 and 1 <= c["stride"] <= 4
            and 1 <= c["g"] <= 8 and all(c[n] % 4 == 0 for n in ("gs", "C", "x0", "x_step")) and c["x0"] >= 0 and c["x_step"] >= 0
            and c["x0"] + (c["g"] - 1) * c["x_step"] + c["gs"] <= c["C"] and c["stride"] * (c["Lout"] - 1) + c["k"] <= c["L"]
            and (c["act"] in (ACT_NONE, ACT_BIAS) or (c["act"] == ACT_BN and c["bn_group"] > 0 and c["C"] % c["bn_group"] == 0))
            and (c["w_group_stride"] == 0 or c["w_group_stride"] >= c["k"] * c["gs"]))


def desc_fields(c):
    return [(n, c[n]) for n in DESC_MEMBERS]


def wstride(c):
    return c["w_group_stride"] or c["k"] * c["gs"]


# ---- the planner of the weight gradient, as csrc/gdwconv.hip plans it ------------------------------------------------------------
def part_rows(c):
    M = c["B"] * c["Lout"]
    col_tiles = -(-(c["g"] * c["gs"] // 4) // 64)
    max_p = max(1, 1024 // col_tiles)
    chunk = max(16, -(-(-(-M // max_p)) // 4) * 4)
    return -(-M // chunk)


def workspace_floats(c):
    return part_rows(c) * (c["k"] + 1) * c["g"] * c["gs"] if in_domain(c) else 0


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def inputs(name):
    c = CASES[name]
    rng = np.random.RandomState(100 + c["seed"])
    B, L, C, g, gs, k, Lout = (c[n] for n in ("B", "L", "C", "g", "gs", "k", "Lout"))
    r = {"x": rng.randint(-3, 4, size=(B, L, C)).astype(np.float32),
         "w": [rng.randint(-2, 3, size=(k, gs)).astype(np.float32) for _ in range(g)],
         "dz": rng.randint(-3, 4, size=(B, Lout, g * gs)).astype(np.float32), "tab": None}
    if c["act"] == ACT_BN:
        bg = c["bn_group"]
        tab = np.full((C // bg, 4, bg), SLACK, np.float32)                # mean and rstd rows: never read
        tab[:, 0] = rng.choice([0.5, 1.0, 2.0, -1.0], size=(C // bg, bg))
        tab[:, 1] = rng.randint(-2, 5, size=(C // bg, bg))
        sc, sh = tab[:, 0].reshape(C), tab[:, 1].reshape(C)
        # a fifth of the elements sit exactly on the kinks: pre = 0 and pre = 6 (scale a power of two: x stays a short dyadic)
        on0, on6 = rng.rand(B, L, C) < 0.1, rng.rand(B, L, C) < 0.1
        r["x"] = np.where(on0, (0 - sh) / sc, np.where(on6, (6 - sh) / sc, r["x"])).astype(np.float32)
        pre = r["x"].astype(np.float64) * sc + sh
        assert (pre == 0).any() and (pre == 6).any() and (pre < 0).any() and (pre > 6).any()
        r["tab"] = tab
    elif c["act"] == ACT_BIAS:
        r["tab"] = rng.randint(-2, 3, size=C).astype(np.float32)
    return r


def activated(c, r):
    x = r["x"].astype(np.float64)
    if c["act"] == ACT_BN:
        C = c["C"]
        return np.clip(x * r["tab"][:, 0].reshape(C).astype(np.float64) + r["tab"][:, 1].reshape(C).astype(np.float64), 0, 6)
    if c["act"] == ACT_BIAS:
        return x + r["tab"].astype(np.float64)
    return x


_REFS = {}


def reference(name):
    """-> the inputs plus float64 Z [B, Lout, g * gs], dA [B, L, C], dw (per group [k, gs]) and dbias [C]; computed once"""
    if name in _REFS:
        return _REFS[name]
    c = CASES[name]
    r = inputs(name)
    A = activated(c, r)
    g, gs, k, s, Lout = c["g"], c["gs"], c["k"], c["stride"], c["Lout"]
    reach = s * (Lout - 1) + 1
    dz = r["dz"].astype(np.float64)
    Z, dA, dw = np.zeros(dz.shape), np.zeros(A.shape), []
    for q in range(g):
        lo = c["x0"] + q * c["x_step"]
        w = r["w"][q].astype(np.float64)
        dzq = dz[:, :, q * gs:(q + 1) * gs]
        dwq = np.zeros((k, gs))
        for j in range(k):
            win = A[:, j:j + reach:s, lo:lo + gs]
            Z[:, :, q * gs:(q + 1) * gs] += w[j] * win
            dA[:, j:j + reach:s, lo:lo + gs] += w[j] * dzq
            dwq[j] = (win * dzq).sum(axis=(0, 1))
        dw.append(dwq)
    r.update(Z=Z, dA=dA, dw=dw, dbias=dA.sum(axis=(0, 1)))
    for v in r.values():
        for a in (v if isinstance(v, list) else [v]):
            if a is not None:
                a.setflags(write=False)
    _REFS[name] = r
    return r
