#!/usr/bin/env python3
"""
Fixture g17_icm_identity, recorded from the *unmodified* reference (build machine only; the import recipe is
tests/golden/ref_import.py): its ICM (networks/ppo_networks/icm.py:22-430) built with encoded_obs_dim = 0, so that there
is no observation encoder and both models work on the flattened observations themselves -- the form
abmarl_blind_maze and robot_warehouse configure.  As g10_icm (make_golden_update.py: gen_g10_icm): ICM.forward on n = 40
rows and the gradients of the training loss ppo.py:2547-2548 at icm_beta = 0.8 w.r.t. every parameter.

  disc   O 2,  Discrete(5), Mi = Mf = 32, depths 2 / 2
  cont   O 17, Box(6),      Mi 64, Mf 32, depths 3 / 1

  <tag>_p_<name>                   parameters (state dict)
  <tag>_names                      parameter names in module order
  <tag>_obs1, _obs2, _actions      inputs
  <tag>_intr                       intrinsic reward [n]
  <tag>_losses                     inverse loss, forward loss, (1 - 0.8) forward + 0.8 inverse
  <tag>_g_<name>                   gradient of that loss

Usage:  python tests/golden/make_golden_icm_identity.py
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402


def gen_g17_icm_identity():
    from ppo_and_friends.networks.ppo_networks.icm import ICM
    from gymnasium.spaces import Box, Discrete
    out = {}
    for tag, (O, space, kw) in {
            "disc": (2, Discrete(5), dict(encoded_obs_dim=0, inverse_hidden_size=32, forward_hidden_size=32)),
            "cont": (17, Box(-1.0, 1.0, (6,), np.float32), dict(encoded_obs_dim=0, inverse_hidden_size=64, forward_hidden_size=32,
                                                                inverse_hidden_depth=3, forward_hidden_depth=1))}.items():
        torch.manual_seed(10)
        icm = ICM(obs_space=Box(-np.inf, np.inf, (O,), np.float32), action_space=space, name="icm", **kw)
        assert not isinstance(icm.obs_encoder, torch.nn.Module)          # the reference's identity: a plain function
        n = 40
        o1, o2 = torch.randn(n, O), torch.randn(n, O)
        act = torch.randint(0, 5, (n, 1)) if tag == "disc" else torch.tanh(torch.randn(n, 6))
        intr, inv_loss, f_loss = icm(o1, o2, act)
        loss = (1.0 - 0.8) * f_loss + 0.8 * inv_loss
        grads = torch.autograd.grad(loss, list(icm.parameters()))
        for k, v in icm.state_dict().items():
            out[f"{tag}_p_{k}"] = v.detach().numpy().copy()
        out[f"{tag}_names"] = np.array([k for k, _ in icm.named_parameters()])
        for (k, _), gr in zip(icm.named_parameters(), grads):
            out[f"{tag}_g_{k}"] = gr.numpy()
        out.update({f"{tag}_obs1": o1.numpy(), f"{tag}_obs2": o2.numpy(), f"{tag}_actions": act.numpy(),
                    f"{tag}_intr": intr.detach().numpy(), f"{tag}_losses": np.array([inv_loss.item(), f_loss.item(), loss.item()])})
    return out


def main():
    scratch = ref_import.make_scratch()
    try:
        out = gen_g17_icm_identity()
    finally:
        ref_import.drop_scratch(scratch)
    path = os.path.join(HERE, "g17_icm_identity.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {len(out)} arrays")


if __name__ == "__main__":
    main()
