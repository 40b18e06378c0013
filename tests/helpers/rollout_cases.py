"""
The rollout-side kernels K1 (csrc/gae.hip), K13 (csrc/env_filters.hip) and K23 (csrc/rollout_finish.hip) restated, and the
cases tests/test_gpu_rollout_kernels_float64.py runs them at.  tests/test_rollout_kernels_oracle.py holds the restatements
to oracle/episode_info_oracle.py, the C oracle, fixtures g1 / g2, oracle/filter_oracle.py and the torch statements of
tests/test_gpu_rollout_finish.py, and asserts, on the reference alone, every condition a case relies on.

K1.  Both recurrences in float64, serial over time and vectorised over the columns:
    adv: A_t = delta_t + gl A_{t+1},  delta_t = r_t + f64(f32(gamma) * Vn_t) - V_t,  gl = gamma * lambda
    rtg: R_t = r_t + gamma R_{t+1}
An end after step t cuts both: Vn_t is the ending value (0 at a terminal end), A_{t+1} := 0 and R_{t+1} := clip(ending
reward), clip(0) at a terminal end; the clip bounds are float32.  The kernel computes in float64 too and rounds once on
output, so the bound per element is derived, not the project's 1e-5 rule:
    2^-23 |x64|                  the final float32 rounding, half an ulp doubled
  + f64_sum_bound(n, S)          n the number of steps to the end of the element's segment (+ 1 for rtg: its seed), S the
                                 same recurrence on absolute values: S_t = |delta_t| + gl S_{t+1} for adv, S_t = |r_t| +
                                 gamma S_{t+1} seeded with |clip(er)| for rtg.
x_t = sum_k g^k term_{t+k} is a sum of n terms; every evaluation order of the chain -- serial, or chunks folded to affine
maps X -> B + M X and composed, as the device does -- rounds each partial sum and each product of g's once, at most about
2 n roundings of relative size 2^-53 on quantities no larger than S, so two orders differ by less than 4 n 2^-53 S;
f64_sum_bound is twice that.  With use_gae = 0, adv is float32(R - v): the rtg bound plus 2^-23 |R - v|.  No element is left
out: the recurrences have no discrete decision.

K13.  The observation streams: batch moments per rank in float64, merged across the rank records with Chan's formula in
rank order and integrated with the step primitive_cases restates for K5, then (x - mean) / sqrt(var + eps) and the clip;
float64 run the reference, float32 run of the same text the floor (eval_kernels.k12_bound).  The reward stream: the
procedure of quirk Q3 itself -- n sequential updates of the half-advanced running-reward vectors, each a Chan merge of the
whole gathered vector (oracle/filter_oracle.py) -- not the pooled S1 / S2 identity the kernel uses.  Its float64 state has a
derived bound: S1 and S2 are sums of N = n * n_all pooled terms, b1 = f64_sum_bound(N, sum w |d|), b2 = f64_sum_bound(N, S2);
to first order mean' = m + S1 / count' moves by b1 / count', var' = (count var + S2 - S1^2 / count') / count' by
(b2 + 2 |S1| b1 / count') / count'; 2^-50 of the value covers the handful of roundings outside the sums, and the bounds of
consecutive steps add, the state before entering the state after with its share count / count' (and the mean's error
moving var' by 2 |mean' - m| times that share of it).

K23.  numpy float32: `r * w` and `+ intrinsic` are two roundings; ends and ep_ts are integers; compared bit for bit.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(os.path.dirname(_HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import primitive_cases as P  # noqa: E402
from primitive_cases import c32, f64_sum_bound, frac, frac_abs  # noqa: E402,F401

F32 = np.float32
U23 = 2.0 ** -23

# ============================================================================================================== K1
# The four instantiations ppoaf_gae_rtg_tmajor chooses among (gae.hip: the launch at the end of the file).  cols: env
# columns of a workgroup; chunk: steps a lane holds at once (TC of the chunked kernel, U of the streaming kernel); tile:
# steps a workgroup covers before it carries over (CW * TS * TC; the streaming kernels carry in registers: None).
INST = {
    "chunk16": dict(cols=16, chunk=4, tile=128, E=(1, 15, 16, 17, 8191), T=(1, 3, 4, 5, 127, 128, 129, 257)),
    "chunk32": dict(cols=32, chunk=8, tile=128, E=(8192, 8193, 8223), T=(1, 7, 8, 9, 128, 129, 257)),
    "stream1": dict(cols=256, chunk=8, tile=None, E=(2 ** 17, 2 ** 17 + 255, 2 ** 17 + 257, 2 ** 20 + 1, 2 ** 20 + 2, 2 ** 20 + 3),
                    T=(1, 7, 8, 9, 17)),
    "stream4": dict(cols=4096, chunk=1, tile=None, E=(2 ** 20, 2 ** 20 + 4, 2 ** 20 + 4100), T=(1, 2, 5)),
}


def instantiation(E, aligned16=True):
    """The kernel the host launches for E columns (aligned16: every array starts on a 16-byte boundary)."""
    if E >= 2 ** 20 and E % 4 == 0 and aligned16:
        return "stream4"
    if E >= 2 ** 17:
        return "stream1"
    return "chunk32" if E >= 8192 else "chunk16"


GAMMA_LAMBDA = [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.5, 0.99)]
CLIPS = [None, (-0.5, 0.5), (0.25, 2.0)]
PATTERNS = ["chunk_first", "chunk_last", "tile_first", "tile_last", "consecutive", "every", "none", "alternating"]
DENSITIES = (0.02, 0.3)


def _tmajor_cases():
    out = []

    def add(inst, E, T, dense, k=None):
        i = len(out)
        k = i // 2 + i // 16 if k is None else k   # walks the patterns and the parameter sets within either form
        gamma, lambd = GAMMA_LAMBDA[(k + i % 2) % 4]
        out.append(dict(name=f"{inst}_E{E}_T{T}_{'dense' if dense else 'fixed'}", inst=inst, E=E, T=T, dense=dense, gamma=gamma,
                        lambd=lambd, clip=CLIPS[(k + i % 2) % 3], use_gae=k % 5 != 2, density=DENSITIES[k % 7 < 3], rot=k, seed=100 + i))
    for inst in ("chunk16", "chunk32"):                      # small: every E with every T, in both forms
        for iE, E in enumerate(INST[inst]["E"]):
            for iT, T in enumerate(INST[inst]["T"]):
                add(inst, E, T, True, iT + 3 * iE)           # every pattern comes to every steered column over the Ts and Es
                add(inst, E, T, False, iT + 3 * iE)
    # large: every E and every T once or more, the longer T at the smaller E, the forms in turn
    for k, (E, T, dense) in enumerate(((2 ** 17, 17, True), (2 ** 17 + 255, 9, False), (2 ** 17 + 257, 8, True), (2 ** 17 + 255, 7, True),
                                      (2 ** 17, 1, False), (2 ** 20 + 1, 7, False), (2 ** 20 + 2, 1, True), (2 ** 20 + 3, 9, True))):
        add("stream1", E, T, dense, k)
    for k, (E, T, dense) in enumerate(((2 ** 20, 5, True), (2 ** 20 + 4, 2, False), (2 ** 20 + 4100, 5, True), (2 ** 20 + 4, 1, True),
                                      (2 ** 20 + 4100, 2, False))):
        add("stream4", E, T, dense, k)
    return out


TMAJOR_CASES = _tmajor_cases()
# E = 2^20, T = 3 with one array 4 bytes (end_kind: 1 and 4 bytes) off a 16-byte boundary: the host routes these to stream1
MISALIGNED = [("rewards", 4), ("values", 4), ("adv_out", 4), ("rtg_out", 4), ("end_kind", 1), ("end_kind", 4)]
MISALIGNED_CASE = dict(name="misaligned", inst="stream1", E=2 ** 20, T=3, dense=True, gamma=0.99, lambd=0.95, clip=(-0.5, 0.5),
                       use_gae=True, density=0.3, rot=3, seed=77)


def chosen_columns(E, cols):
    """The steered columns: column 0, the first and last column of a workgroup (of the first, the second, the last full
    and the last one), and column E - 1 (in a ragged last workgroup where E % cols != 0)."""
    nwg = -(-E // cols)
    c = {0, min(cols - 1, E - 1), E - 1, (nwg - 1) * cols}
    if nwg > 1:
        c |= {cols, min(2 * cols - 1, E - 1), (nwg - 1) * cols - 1}
    return sorted(c)


def steered_ends(pattern, T, chunk, tile):
    """end_kind [T] of one steered column, before the last row is closed.  `back` counts steps from the end of the rollout
    (1: the last row): chunks and tiles are laid out from there."""
    t = np.arange(T)
    back = T - t
    m = np.zeros(T, bool)
    if pattern == "chunk_first":
        m = (back % chunk == 0) & ((back // chunk) % 2 == 1)
    elif pattern == "chunk_last":
        m = ((back - 1) % chunk == 0) & (((back - 1) // chunk) % 2 == 1)
    elif pattern == "tile_first" and tile:
        m = back % tile == 0
    elif pattern == "tile_last" and tile:
        m = ((back - 1) % tile == 0) & (back > 1)
    elif pattern == "consecutive" and T >= 3:
        m[T // 2 - 1:T // 2 + 1] = True
    elif pattern in ("every", "alternating"):
        m[:] = True
    kind = np.where(m, 2 if pattern == "every" else 1 + t % 2, 0)
    return kind.astype(np.int8)


def column_patterns(c):
    """{column: pattern} of a dense case."""
    inst = INST[c["inst"]]
    pats = [p for p in PATTERNS if inst["tile"] or not p.startswith("tile")]         # the streaming kernels have no tile
    return {col: pats[(j + c["rot"]) % len(pats)] for j, col in enumerate(chosen_columns(c["E"], inst["cols"]))}


def tmajor_inputs(c):
    """float32 rewards U(-1, 1), values N(0, 1), ending values N(0, 2); ending rewards half N(0, 100) (the clip bites), half
    U(-1, 3) (it does not always); dense form: [T, E] tables and end_kind, the steered columns as column_patterns says, the
    rest ended at random with the case's density, kinds 1 and 2 alike, the last row closed with kind 2."""
    T, E = c["T"], c["E"]
    rng = np.random.default_rng(c["seed"])
    f = lambda *s: rng.standard_normal(s, dtype=F32)
    rew = (rng.random((T, E), dtype=F32) * F32(2) - F32(1))
    val = f(T, E)
    shape = (T, E) if c["dense"] else (E,)
    bv = f(*shape) * F32(2)
    br = np.where(rng.random(shape, dtype=F32) < 0.5, f(*shape) * F32(100), rng.random(shape, dtype=F32) * F32(4) - F32(1)).astype(F32)
    ekd = None
    if c["dense"]:
        u = rng.random((T, E), dtype=F32)
        p = c["density"]
        ekd = np.where(u < p / 2, 1, np.where(u < p, 2, 0)).astype(np.int8)
        inst = INST[c["inst"]]
        for col, pat in column_patterns(c).items():
            ekd[:, col] = steered_ends(pat, T, inst["chunk"], inst["tile"])
        ekd[-1] = np.where(ekd[-1] == 0, 2, ekd[-1])
    return dict(rew=rew, val=val, bv=bv, br=br, ek=ekd)


def clip32(x, clip):
    x = np.asarray(x, F32)
    return x if clip is None else np.clip(x, F32(clip[0]), F32(clip[1]))


def gae_terms(rew, val, bv, br, ekd, gamma, clip):
    """Per step [T, E]: delta (float64), ends (bool), the rtg seed clip(ending reward) (float64, read where ends).
    ekd None: the fixed-length form, one bootstrapped end after the last row, bv / br [E]."""
    T, E = rew.shape
    if ekd is None:
        kind = np.zeros((T, E), np.int8)
        kind[-1] = 2
        bvt, brt = np.zeros((T, E), F32), np.zeros((T, E), F32)
        bvt[-1], brt[-1] = bv, br
    else:
        kind, bvt, brt = ekd, bv, br
    vnext = np.concatenate([val[1:], np.zeros((1, E), F32)], 0)
    vn = np.where(kind == 2, bvt, np.where(kind == 1, F32(0), vnext)).astype(F32)
    gv = F32(gamma) * vn                                                 # a float32 product, widened afterwards
    assert gv.dtype == F32
    delta = rew.astype(np.float64) + gv.astype(np.float64) - val.astype(np.float64)
    seed = clip32(np.where(kind == 2, brt, F32(0)), clip).astype(np.float64)
    return delta, kind != 0, seed


def gae_tmajor_ref(rew, val, bv, br, ekd, gamma, lambd, clip, use_gae):
    """-> dict(adv, rtg: float64 [T, E]; adv_bound, rtg_bound: the module docstring's bound per element)."""
    T, E = rew.shape
    delta, ends, seed = gae_terms(rew, val, bv, br, ekd, gamma, clip)
    gl = float(gamma) * float(lambd)
    r64 = rew.astype(np.float64)
    A, R, SA, SR, n = (np.zeros(E) for _ in range(5))
    out = {k: np.empty((T, E)) for k in ("adv", "rtg", "adv_bound", "rtg_bound")}
    for t in range(T - 1, -1, -1):
        e = ends[t]
        A = delta[t] + np.where(e, 0.0, gl * A)
        SA = np.abs(delta[t]) + np.where(e, 0.0, gl * SA)
        R = r64[t] + gamma * np.where(e, seed[t], R)
        SR = np.abs(r64[t]) + gamma * np.where(e, np.abs(seed[t]), SR)
        n = np.where(e, 1.0, n + 1.0)
        out["rtg"][t] = R
        out["rtg_bound"][t] = U23 * np.abs(R) + f64_sum_bound(n + 1.0, SR)
        if use_gae:
            out["adv"][t] = A
            out["adv_bound"][t] = U23 * np.abs(A) + f64_sum_bound(n, SA)
        else:
            out["adv"][t] = R - val[t].astype(np.float64)
            out["adv_bound"][t] = out["rtg_bound"][t] + U23 * np.abs(out["adv"][t])
    return out


def gae_tmajor_composed(rew, val, bv, br, ekd, gamma, lambd, clip, chunk, tile):
    """The same two chains in float64 in the device's evaluation order: every chunk of `chunk` steps folded to the affine
    maps X -> B + M X, the maps of a tile composed latest first, every chunk replayed from the composed carry, the tile's
    whole map applied to the carry of the tile before.  -> (adv, rtg) float64, use_gae = 1."""
    T, E = rew.shape
    delta, ends, seed = gae_terms(rew, val, bv, br, ekd, gamma, clip)
    gl, r64 = float(gamma) * float(lambd), rew.astype(np.float64)
    tile = tile or T
    adv, rtg = np.empty((T, E)), np.empty((T, E))
    carryA, carryR = np.zeros(E), np.zeros(E)
    then = lambda f, s: (s[0] * f[0], s[1] + s[0] * f[1], s[2] * f[2], s[3] + s[2] * f[3])      # (Ma, Ba, Mr, Br)
    for t_hi in range(T, 0, -tile):
        run = (np.ones(E), np.zeros(E), np.ones(E), np.zeros(E))
        for c in range(-(-tile // chunk)):
            c_hi = t_hi - c * chunk
            c_lo = max(c_hi - chunk, 0)
            if c_hi <= c_lo:
                break
            Ma, Ba, Mr, Br = np.ones(E), np.zeros(E), np.ones(E), np.zeros(E)
            A, R = run[1] + run[0] * carryA, run[3] + run[2] * carryR
            for t in range(c_hi - 1, c_lo - 1, -1):
                e = ends[t]
                Ba, Ma = delta[t] + np.where(e, 0.0, gl * Ba), np.where(e, 0.0, gl * Ma)
                Br, Mr = r64[t] + gamma * np.where(e, seed[t], Br), np.where(e, 0.0, gamma * Mr)
                A = delta[t] + np.where(e, 0.0, gl * A)
                R = r64[t] + gamma * np.where(e, seed[t], R)
                adv[t], rtg[t] = A, R
            run = then(run, (Ma, Ba, Mr, Br))
        carryA, carryR = run[1] + run[0] * carryA, run[3] + run[2] * carryR
    return adv, rtg


def chunk_edges(T, chunk, tile):
    """Which steps are the first / last of a lane chunk and of a tile, walked as the kernel walks them:
    dict(chunk_first, chunk_last, tile_first, tile_last) of bool [T]."""
    tile = tile or T
    o = {k: np.zeros(T, bool) for k in ("chunk_first", "chunk_last", "tile_first", "tile_last")}
    for t_hi in range(T, 0, -tile):
        o["tile_last"][t_hi - 1] = True
        o["tile_first"][max(t_hi - tile, 0)] = True
        for c in range(-(-tile // chunk)):
            c_hi = t_hi - c * chunk
            c_lo = max(c_hi - chunk, 0)
            if c_hi > c_lo:
                o["chunk_first"][c_lo], o["chunk_last"][c_hi - 1] = True, True
    return o


# ---- trajectory form
TRAJ_CASES = [
    dict(name="n1", lens=[1000], gamma=0.99, lambd=0.95, clip=(-0.5, 0.5), use_gae=True, rtg=True),
    dict(name="n3_zero_mid", lens=[63, 0, 64], gamma=1.0, lambd=1.0, clip=None, use_gae=True, rtg=False),
    dict(name="n4", lens=[65, 128, 1, 129], gamma=0.9, lambd=0.0, clip=(0.25, 2.0), use_gae=False, rtg=True),
    dict(name="n5_zero_mid", lens=[1, 64, 0, 129, 63], gamma=0.5, lambd=0.99, clip=(-0.5, 0.5), use_gae=True, rtg=False),
    dict(name="n9_zero_mid", lens=[1000, 1, 63, 64, 0, 65, 128, 129, 1], gamma=0.99, lambd=0.95, clip=(0.25, 2.0), use_gae=True, rtg=True),
]
TRAJ_GAP = 5


def traj_inputs(c):
    """The trajectories laid into one flat buffer in a shuffled order with TRAJ_GAP elements before, between and after
    them, so that the start table is not in address order.  -> dict(rew, val, ev, er, start, lens, N, used (bool [N]))."""
    lens = np.array(c["lens"], np.int32)
    n = len(lens)
    rng = np.random.default_rng(1000 + n)
    order = rng.permutation(n) if n > 1 else np.arange(1)
    if n > 1 and (np.diff(order) > 0).all():
        order = order[::-1]
    start, pos = np.zeros(n, np.int64), TRAJ_GAP
    for k in order:
        start[k] = pos
        pos += int(lens[k]) + TRAJ_GAP
    N = pos
    used = np.zeros(N, bool)
    for s, L in zip(start, lens):
        used[s:s + L] = True
    rew = (rng.random(N, dtype=F32) * F32(2) - F32(1))
    val = rng.standard_normal(N, dtype=F32)
    ev = rng.standard_normal(n, dtype=F32) * F32(2)
    er = np.where(np.arange(n) % 2 == 0, rng.standard_normal(n) * 100, rng.uniform(-1, 3, n)).astype(F32)
    return dict(rew=rew, val=val, ev=ev, er=er, start=start, lens=lens, N=N, used=used)


def gae_traj_ref(inp, c):
    """gae_tmajor_ref per trajectory (one column, the fixed-length form) -> the same dict over the flat buffer, NaN and a
    zero bound in the gaps."""
    out = {k: np.full(inp["N"], np.nan) for k in ("adv", "rtg")}
    out.update({k: np.zeros(inp["N"]) for k in ("adv_bound", "rtg_bound")})
    for i, (s, L) in enumerate(zip(inp["start"], inp["lens"])):
        if L == 0:
            continue
        sl = slice(s, s + L)
        r = gae_tmajor_ref(inp["rew"][sl, None], inp["val"][sl, None], inp["ev"][i:i + 1], inp["er"][i:i + 1], None, c["gamma"],
                           c["lambd"], c["clip"], c["use_gae"])
        for k in out:
            out[k][sl] = r[k][:, 0]
    return out


# ============================================================================================================== K13
K13_DEFAULTS = dict(G=1, W=1, streams="ocr", data="std", reward="std", done2=True, gamma=0.97, clip=None, rclip=None, normalize=True,
                    frozen="", ranks=None, zero_record=False, steps=3)
K13_CASES = [
    # n = 1: from the initial count of 1e-4 the float32 mean lies within 1e-4 |x| of x, so x - mean is left with a relative
    # error of 6e-4 in any float32 arithmetic: the observation streams normalise from n = 2 on, clip at n = 1
    dict(name="n1_reward_only", n=1, G=3, streams="r", rclip=(-0.6, 0.9)),
    dict(name="n1_clip_only", n=1, G=3, W=17, normalize=False, clip=(-0.5, 0.5), rclip=(-0.2, 0.3)),
    dict(name="n2_G3_W17_far", n=2, G=3, W=17, data="far"),
    dict(name="n63_reward_only_far", n=63, W=17, streams="r", reward="far", done2=False, gamma=1.0),
    dict(name="n64_critic_only_tiny", n=64, G=3, streams="c", data="tiny"),
    dict(name="n65_obs_reward", n=65, streams="or", rclip=(-0.4, 0.7)),
    dict(name="n255_G3_W17_far", n=255, G=3, W=17, data="far", reward="far"),
    dict(name="n256_W17_tiny", n=256, W=17, data="tiny", gamma=1.0, done2=False),
    dict(name="n257_G3_clip", n=257, G=3, clip=(-1.0, 1.5), rclip=(-0.5, 0.25)),
    dict(name="n1000_W17_far", n=1000, W=17, data="far"),
    dict(name="n1000_G3_reward_only", n=1000, G=3, streams="r"),
    dict(name="n65_G3_W17_obs_frozen", n=65, G=3, W=17, frozen="oc"),
    dict(name="n257_all_frozen", n=257, frozen="ocr", data="far", reward="far"),
    dict(name="n257_G3_W17_clip_only", n=257, G=3, W=17, normalize=False, clip=(-0.5, 0.5), rclip=(-0.2, 0.3)),
    dict(name="n64_W17_clip_lo_eq_hi", n=64, W=17, clip=(0.25, 0.25), rclip=(0.125, 0.125)),
    dict(name="R3_unequal_n_obs", n=64, G=3, W=17, streams="oc", ranks=(64, 1, 257), data="far"),
    dict(name="R3_unequal_n_zero_record", n=255, W=1, streams="o", ranks=(255, 0, 2)),
    dict(name="R3_equal_n", n=65, G=3, W=17, ranks=(65, 65, 65), reward="far"),
    dict(name="R3_equal_n_zero_record", n=256, G=1, W=1, ranks=(256, 0, 256), done2=False),
]
K13_EPS = 1e-8
DATA = dict(std=(0.0, 1.0), far=(1000.0, 1.0), tiny=(0.0, 1e-3))
REWARD = dict(std=(0.0, 1.0), far=(20.0, 2.0))


def k13_case(c):
    c = {**K13_DEFAULTS, **c}
    c["ranks"] = tuple(c["ranks"] or (c["n"],))          # rows per rank; 0: a rank without rows (an all-zero record)
    assert c["ranks"][0] == c["n"]
    return c


def k13_inputs(c):
    """Per step and per rank with rows: x / cx [G * n_r, W] float32 (agent-major rows), reward [G * n_r] float32,
    terminated and truncated bool [G * n_r]."""
    c = k13_case(c)
    rng = np.random.default_rng(c["n"] * 31 + c["G"] * 7 + c["W"])
    mu, sd = DATA[c["data"]]
    rmu, rsd = REWARD[c["reward"]]
    steps = []
    for _ in range(c["steps"]):
        ranks = []
        for nr in c["ranks"]:
            if nr == 0:
                ranks.append(None)
                continue
            rows = c["G"] * nr
            # every agent and feature with a mean and a scale of its own around the case's
            x, cx = ((mu + sd * (1.0 + 0.1 * np.arange(c["W"])) * rng.standard_normal((rows, c["W"])) + sd * np.arange(c["W"])).astype(F32)
                     for _ in range(2))
            ranks.append(dict(o=x, c=cx, r=(rmu + rsd * rng.standard_normal(rows)).astype(F32),
                              term=rng.random(rows) < 0.2, trunc=rng.random(rows) < 0.2))
        steps.append(ranks)
    return steps


def obs_records(x, G):
    """x [G * n, W] -> float64 (mean [G, W], M2 [G, W]) of every agent's rows."""
    x = np.asarray(x, np.float64).reshape(G, -1, x.shape[-1])
    mean = x.mean(1)
    return mean, ((x - mean[:, None]) ** 2).sum(1)


class ObsStreamRef:
    """One observation stream of all ranks (they share the statistics): mean / var [G, W] in `dtype`, count [G]."""

    def __init__(self, G, W, dtype):
        self.G, self.W, self.dtype = G, W, dtype
        self.mean, self.var, self.count = np.zeros((G, W), dtype), np.ones((G, W), dtype), np.full(G, 1e-4)

    def step(self, xs, update, normalize, clip, zero_record=False):
        """xs: the ranks' batches (None: a rank without rows).  -> the filtered batch of rank 0."""
        G, W, dt = self.G, self.W, self.dtype
        x0 = xs[0].reshape(G, -1, W)
        if normalize and update:
            recs = [(float(x.shape[0] // G),) + obs_records(x, G) if x is not None else None for x in xs]
            for g in range(G):
                rows = np.array([np.zeros(1 + 2 * W) if r is None else np.concatenate([[r[0]], r[1][g], r[2][g]]) for r in recs])
                self.mean[g], self.var[g], self.count[g] = P.integrate_ref(rows, self.mean[g], self.var[g], self.count[g], dt)
        out = np.empty(x0.shape, dt)
        for g in range(G):
            y = P.normalize_ref(x0[g], self.mean[g], self.var[g], None, dt, K13_EPS) if normalize else x0[g].astype(dt)
            out[g] = y if clip is None else np.clip(y, dt(F32(clip[0])), dt(F32(clip[1])))
        return out.reshape(-1, W)


class RewardStreamRef:
    """The reward stream of all ranks with rows: running_reward [R][G, n], mean / var / count [G], all float64 (the
    reference's float32 scalars are promoted by the first float64 batch), with the bounds of the module docstring
    accumulated over the steps; the output in `dtype`."""

    def __init__(self, G, n, R, gamma, dtype):
        self.G, self.n, self.R, self.gamma, self.dtype = G, n, R, float(gamma), dtype
        self.rr = np.zeros((R, G, n))
        self.mean, self.var, self.count = np.zeros(G), np.ones(G), np.full(G, 1e-4)
        self.b_rr, self.b_mean, self.b_var = np.zeros((R, G, n)), np.zeros(G), np.zeros(G)

    def step(self, rews, dones, update, normalize, clip):
        """rews / dones [R][G * n].  -> the filtered rewards of rank 0."""
        G, n, R, dt = self.G, self.n, self.R, self.dtype
        rew = np.stack([np.asarray(r, np.float64).reshape(G, n) for r in rews])             # [R, G, n]
        if normalize and update:
            for g in range(G):
                m0, c0, v0 = self.mean[g], self.count[g], self.var[g]
                old, new = self.rr[:, g].copy(), self.rr[:, g] * self.gamma + rew[:, g]
                vec = self.rr[:, g]                                       # advanced in place, env by env
                for e in range(n):                                        # filter_wrappers.py:412-418 (Q3)
                    vec[:, e] = vec[:, e] * self.gamma + rew[:, g, e]
                    bm, bvar, N = vec.mean(), vec.var(), float(vec.size)
                    delta = bm - self.mean[g]                             # stats.py:73-94
                    new_count = self.count[g] + N
                    self.mean[g] = self.mean[g] + delta * (N / new_count)
                    m_2 = self.var[g] * self.count[g] + bvar * N + np.square(delta) * self.count[g] * N / (self.count[g] + N)
                    self.var[g] = m_2 / (self.count[g] + N)
                    self.count[g] += N
                # the bound: the pooled terms, weight n - i on the advanced value of env i, i on the one before
                w1, w0 = (n - np.arange(n))[None, :], np.arange(n)[None, :]
                d1, d0 = new - m0, old - m0
                S1abs, S2 = (w1 * np.abs(d1) + w0 * np.abs(d0)).sum(), (w1 * d1 * d1 + w0 * d0 * d0).sum()
                S1, N, cnt = (w1 * d1 + w0 * d0).sum(), float(n) * n * R, self.count[g]
                b1, b2 = f64_sum_bound(N, S1abs), f64_sum_bound(N, S2)
                keep = c0 / cnt                                           # the share of the state before in the state after
                self.b_var[g] = (keep * self.b_var[g] + 2.0 * abs(self.mean[g] - m0) * keep * self.b_mean[g]
                                 + (b2 + 2.0 * abs(S1) * b1 / cnt) / cnt + 2.0 ** -50 * (c0 * v0 + S2) / cnt)
                self.b_mean[g] = keep * self.b_mean[g] + b1 / cnt + 2.0 ** -50 * abs(self.mean[g])
                self.b_rr[:, g] = self.gamma * self.b_rr[:, g] + 4 * 2.0 ** -53 * (np.abs(old) * self.gamma + np.abs(rew[:, g]))
        out = rew[0].astype(dt)
        if normalize:
            done = np.stack([np.asarray(d, bool).reshape(G, n) for d in dones])
            self.rr[done], self.b_rr[done] = 0.0, 0.0
            out = out / np.sqrt(self.var.astype(dt) + dt(K13_EPS))[:, None]
        if clip is not None:
            out = np.clip(out, dt(F32(clip[0])), dt(F32(clip[1])))
        return out.reshape(-1)


def k13_reference(c, dtype):
    """The whole case in `dtype`: per step dict(o, c, r: rank 0's outputs; state: copies of the stream states after it)."""
    c = k13_case(c)
    steps = k13_inputs(c)
    G, W = c["G"], c["W"]
    live = [i for i, nr in enumerate(c["ranks"]) if nr > 0]
    obs = {s: ObsStreamRef(G, W, dtype) for s in "oc" if s in c["streams"]}
    rw = RewardStreamRef(G, c["n"], len(live), c["gamma"], dtype) if "r" in c["streams"] else None
    out = []
    for k, ranks in enumerate(steps):
        o = {}
        for s, st in obs.items():
            o[s] = st.step([None if r is None else r[s] for r in ranks], not (s in c["frozen"] and k > 0), c["normalize"], c["clip"])
            o[s + "_state"] = (st.mean.copy(), st.var.copy(), st.count.copy())
        if rw is not None:
            dones = [ranks[i]["term"] | (ranks[i]["trunc"] if c["done2"] else False) for i in live]
            o["r"] = rw.step([ranks[i]["r"] for i in live], dones, not ("r" in c["frozen"] and k > 0), c["normalize"], c["rclip"])
            o["r_state"] = dict(rr=rw.rr[0].copy(), mean=rw.mean.copy(), var=rw.var.copy(), count=rw.count.copy(), b_rr=rw.b_rr[0].copy(),
                                b_mean=rw.b_mean.copy(), b_var=rw.b_var.copy())
        out.append(o)
    return out


# ============================================================================================================== K23
# members of the one launch: (blocks, grouped); 8 members, one with 16 blocks, two grouped with shuffled slot orders
FINISH_MEMBERS = [(16, False), (5, True), (1, False), (2, False), (3, True), (1, False), (4, False), (2, True)]
FINISH_CASES = [
    dict(name="E255", E=255, w=0.37, intrinsic=True, truncated=True, write_ends=True, natural="some", natural_out_null=()),
    dict(name="E256_w1_no_truncated", E=256, w=1.0, intrinsic=True, truncated=False, write_ends=True, natural="some", natural_out_null=()),
    dict(name="E257_no_ends", E=257, w=0.37, intrinsic=False, truncated=True, write_ends=False, natural="none", natural_out_null=()),
    dict(name="E513", E=513, w=0.37, intrinsic=True, truncated=True, write_ends=True, natural="all", natural_out_null=(2, 4)),
]
FINISH_STEPS, FINISH_MAX_TS = 4, 3


def finish_slot_agent(m, n):
    """A shuffled slot order of grouped member m (never the identity for n > 1)."""
    p = np.random.default_rng(50 + m).permutation(n)
    return p if n == 1 or (p != np.arange(n)).any() else p[::-1].copy()


def finish_inputs(c):
    """Per step: per member reward [n, E] and natural [n, E] float32 U(-1, 1) (natural_given [n]: False = a NULL block),
    intrinsic [n * E] or None (member 0 and 3 never have one), terminated / truncated bool [E]."""
    E, rng = c["E"], np.random.default_rng(c["E"])
    u = lambda *s: (rng.random(s, dtype=F32) * F32(2) - F32(1))
    steps = []
    for t in range(FINISH_STEPS):
        mem = []
        for m, (n, grouped) in enumerate(FINISH_MEMBERS):
            given = np.array([{"all": True, "none": False, "some": (b + m) % 3 != 0}[c["natural"]] for b in range(n)])
            mem.append(dict(reward=u(n, E), natural=u(n, E), natural_given=given,
                            intrinsic=u(n * E) if c["intrinsic"] and m not in (0, 3) else None))
        steps.append(dict(members=mem, term=rng.random(E) < 0.2, trunc=rng.random(E) < 0.2, last=t == FINISH_STEPS - 1))
    return steps


def finish_ref(c, step, ep_ts, outs, members=None, orders=None, max_ts=FINISH_MAX_TS):
    """One launch on numpy float32.  outs: per member dict(reward [n * E] f32, natural [n * E] f32 or None, end_kind int8
    [E] (grouped) or [n * E]) as they were; -> (ep_ts, outs) as the launch leaves them.  members / orders: another member
    list than FINISH_MEMBERS with its slot orders."""
    members = FINISH_MEMBERS if members is None else members
    E, w = c["E"], F32(c["w"])
    ep_ts, kind = ep_ts.copy(), np.zeros(E, np.int8)
    if c["write_ends"]:
        term = step["term"]
        trunc = step["trunc"] if c["truncated"] else np.zeros(E, bool)
        ts = ep_ts + 1
        boot = ~term & ((ts >= max_ts) | trunc | step["last"])
        kind = np.where(term, 1, np.where(boot, 2, 0)).astype(np.int8)
        ep_ts = np.where(term | boot, 0, ts).astype(np.int32)
    new = []
    for m, ((n, grouped), mem, o) in enumerate(zip(members, step["members"], outs)):
        o = {k: None if v is None else v.copy() for k, v in o.items()}
        order = (finish_slot_agent(m, n) if orders is None else np.asarray(orders[m])) if grouped else np.arange(n)
        for s in range(n):
            b = order[s]
            idx = np.arange(E) * n + s if grouped else s * E + np.arange(E)
            r = mem["reward"][b]
            if o["natural"] is not None:
                o["natural"][b * E:(b + 1) * E] = mem["natural"][b] if mem["natural_given"][b] else r
            if w != F32(1.0):
                r = r * w
            if mem["intrinsic"] is not None:
                r = r + mem["intrinsic"][idx]
            assert r.dtype == F32
            o["reward"][idx] = r
            if c["write_ends"] and not grouped:
                o["end_kind"][idx] = kind
        if c["write_ends"] and grouped:
            o["end_kind"][:] = kind
        new.append(o)
    return ep_ts, new


def finish_blank_outs(c):
    """The output rows before the first launch: sentinels (-777 / -7) a launch that skipped an element would leave."""
    E = c["E"]
    return [dict(reward=np.full(n * E, -777.0, F32), natural=None if m in c["natural_out_null"] else np.full(n * E, -777.0, F32),
                 end_kind=np.full(E if grouped else n * E, -7, np.int8)) for m, (n, grouped) in enumerate(FINISH_MEMBERS)]
