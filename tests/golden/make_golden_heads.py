#!/usr/bin/env python3
"""
Fixture g16_action_heads, recorded from the *unmodified* reference (build machine only; the import recipe is
tests/golden/ref_import.py): its MultiCategoricalDistribution (networks/distributions.py:272-438) and
BernoulliDistribution (:134-196), built by get_actor_distribution (:984-1115) together with their output functions --
the per-slice softmax (:1047-1064) and the sigmoid (:1111-1113) -- on fixed logits and actions:

  <tag>_logits, <tag>_actions               inputs: float32 [n, outputs]; int64 [n, D] / float32 [n, bits] of 0 / 1
  <tag>_log_probs, <tag>_entropy            [n] each
  <tag>_dlogp_dlogits, <tag>_dent_dlogits   gradients of their sums w.r.t. the logits
  <tag>_refined                             refine_prediction of the output function's values (the multi-categorical
                                            one row at a time: the reference's fills one slot per action dimension)
  <tag>_nvec                                MultiDiscrete only

The first four rows of every case hold saturated logits (+-16, +-20), so that the probability clamps and their inclusive
bounds (sigmoid(16) rounds to exactly 1 - eps) are exercised.

Usage:  python tests/golden/make_golden_heads.py
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

CASES = {"md34": [3, 4], "md2222": [2, 2, 2, 2], "md13": [1, 3], "mb1": 1, "mb4": 4, "mb8": 8}
SATURATED = (16.0, -16.0, 20.0, -20.0)


def record(tag, spec, g):
    import ppo_and_friends.networks.distributions as D
    from gymnasium.spaces import MultiBinary, MultiDiscrete
    multi = isinstance(spec, list)
    dist, output_func = D.get_actor_distribution(MultiDiscrete(spec) if multi else MultiBinary(spec))
    k, n = (sum(spec) if multi else spec), 20
    logits = torch.randn(n, k, generator=g) * 3.0
    for r in range(4):
        logits[r] = torch.tensor([SATURATED[(r + c) % 4] for c in range(k)])
    if multi:
        actions = torch.stack([torch.randint(0, m, (n,), generator=g) for m in spec], dim=1)
    else:
        actions = torch.randint(0, 2, (n, k), generator=g).float()
    lg = logits.clone().requires_grad_(True)
    td = dist.get_distribution(output_func(lg * 1.0))     # a non-leaf copy: the MultiDiscrete output function writes in place
    lp = dist.get_log_probs(td, actions)
    ent = dist.get_entropy(td)
    glp, = torch.autograd.grad(lp.sum(), lg, retain_graph=True)
    gent, = torch.autograd.grad(ent.sum(), lg)
    with torch.no_grad():
        probs = output_func(logits.clone())
        if multi:
            refined = torch.stack([dist.refine_prediction(probs[r:r + 1].clone()) for r in range(n)])
        else:
            refined = dist.refine_prediction(probs.clone())
    out = {f"{tag}_logits": logits.numpy(), f"{tag}_actions": actions.numpy(), f"{tag}_log_probs": lp.detach().numpy(),
           f"{tag}_entropy": ent.detach().numpy(), f"{tag}_dlogp_dlogits": glp.numpy(), f"{tag}_dent_dlogits": gent.numpy(),
           f"{tag}_refined": refined.numpy()}
    if multi:
        out[f"{tag}_nvec"] = np.asarray(spec, np.int64)
    return out


def main():
    scratch = ref_import.make_scratch()
    try:
        g = torch.Generator().manual_seed(16)
        out = {}
        for tag, spec in CASES.items():
            out.update(record(tag, spec, g))
    finally:
        ref_import.drop_scratch(scratch)
    path = os.path.join(HERE, "g16_action_heads.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {len(out)} arrays")


if __name__ == "__main__":
    main()
