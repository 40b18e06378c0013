"""
The cases of the wide-action form of K14's shapes chain and identity form (csrc/icm_update_shapes.hip: icm_sh_models_kernel
<., 32>, icm_sh_reward_kernel<., 32>; Discrete / Box actions of 9 .. 24 classes or dimensions), shared by
tests/test_gpu_icm_wide_actions_float64.py (the kernels against float64) and tests/test_icm_wide_actions_oracle.py (the
float32 oracle and planted errors against it; no GPU).  Cases, reference and bound are tests/helpers/icm_float64.py's.

The smallest shapes at which the new code can go wrong: A in (9, 16, 17, 24) -- the first width above the 8-wide head, the
edges of the second 16-column K step of the action tile, the form's limit -- Discrete and Box each, on both chains; B = 33
(all 24 classes occur, three tiles, the last one ragged) with one case at 17 and one at 257; the four row addressings; depths
(1, 3) and (3, 1); Mi != Mf in both orders (one launch per model) and Mi == Mf (one launch for both); D in (9, 16, 17); the
three activations; icm_beta 0 and 1 once each; mario_bros_ram's ICM (O 256, E 128, D 9, M 32 / 32, Discrete(18)); and the
default one-width ICM (128 everywhere), which goes to the shapes chain with such actions.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icm_float64 as H  # noqa: E402

WIDE_WIDTHS = (9, 16, 17, 24)
KINDS = ("discrete", "continuous")


def _cases():
    out = {}
    rot = lambda seq, i: seq[i % len(seq)]
    depths = [(1, 3), (3, 1)]
    # (E, Mi, Mf): Mi != Mf in both orders, and one equal pair (both models in one launch)
    triples = [(32, 64, 128), (64, 128, 32), (128, 32, 64), (32, 128, 64), (64, 32, 32), (128, 64, 32), (32, 32, 128), (64, 128, 128)]
    pairs = [(32, 64), (64, 32), (128, 32), (32, 128), (64, 64), (128, 64), (64, 128), (32, 32)]
    i = 0
    for A in WIDE_WIDTHS:
        for kind in KINDS:
            E, Mi, Mf = rot(triples, i)
            out[f"sh_{kind[:4]}{A}"] = H.case("shapes", (10, 23)[i % 2], 33, (E, rot((9, 16, 17), i), Mi, Mf), depths=rot(depths, i),
                                              action=(kind, A), act=rot(H.ACTIVATIONS, i), beta=(0.2, 0.8)[i % 2],
                                              rows=rot(H.ROW_MODES, i), seed=3000 + i)
            out[f"id_{kind[:4]}{A}"] = H.case("identity", rot((5, 16, 17, 40), i), 33, rot(pairs, i), depths=rot(depths, i + 1),
                                              action=(kind, A), act=rot(H.ACTIVATIONS, i + 1), beta=(0.8, 0.2)[i % 2],
                                              rows=rot(H.ROW_MODES, i + 2), seed=3100 + i)
            i += 1
    # batch edges: one tile and a ragged second one (17 classes at most fit), 17 tiles
    out["sh_B17"] = H.case("shapes", 12, 17, (64, 9, 32, 64), depths=(3, 1), action=("discrete", 17), act="tanh", beta=0.2,
                           rows="tail", seed=3201)
    out["id_B17"] = H.case("identity", 12, 17, (64, 32), depths=(1, 3), action=("continuous", 24), act="leaky_relu", beta=0.8,
                           rows="order", seed=3202)
    out["sh_B257"] = H.case("shapes", 12, 257, (32, 17, 64, 32), depths=(1, 3), action=("discrete", 24), beta=0.8, rows="perm",
                            seed=3203)
    out["id_B258"] = H.case("identity", 12, 258, (32, 64), depths=(3, 1), action=("continuous", 17), act="tanh", beta=0.2,
                            rows="agents", seed=3204)
    # mario_bros_ram --enable_icm 1, and the default ICM (one width, 128) over such actions
    out["sh_mario"] = H.case("shapes", 256, 33, (128, 9, 32, 32), depths=(2, 2), action=("discrete", 18), beta=0.2, rows="perm",
                             seed=3301)
    out["sh_default128_box17"] = H.case("shapes", 20, 33, (128, 128, 128, 128), depths=(2, 2), action=("continuous", 17),
                                        beta=0.2, rows="tail", seed=3302)
    out["sh_default128_disc18"] = H.case("shapes", 20, 33, (128, 128, 128, 128), depths=(2, 2), action=("discrete", 18),
                                         act="leaky_relu", beta=0.8, rows="order", seed=3303)
    # icm_beta 0 (the inverse model takes no gradient: exactly zero) and 1 (the forward model)
    out["sh_beta0"] = H.case("shapes", 7, 33, (64, 16, 32, 64), depths=(1, 3), action=("discrete", 24), beta=0.0, rows="agents",
                             seed=3401)
    out["id_beta1"] = H.case("identity", 7, 33, (64, 32), depths=(3, 1), action=("continuous", 9), act="tanh", beta=1.0,
                             rows="perm", seed=3402)
    return out


CASES = _cases()
