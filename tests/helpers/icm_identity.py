"""
The torch-CPU oracle of an ICM with an identity encoder (ICM(encoded_obs_dim = 0), icm.py:326-337): oracle/icm_oracle.ICM
built with an encoding as wide as the observation -- which gives both models their layer sizes -- and its encoder replaced
by nn.Identity().  Shared by tests/test_gpu_icm_identity.py and tests/test_gpu_icm_grouped.py.
"""
import torch.nn as nn

from oracle import cpu_ppo_loop, icm_oracle


def oracle_icm(O, NA, discrete, Mi, Mf, d_inv=2, d_fwd=2, activation="relu"):
    ref = icm_oracle.ICM(O, NA, discrete=discrete, enc=O, hidden=Mi, inv_depth=d_inv, fwd_depth=d_fwd, activation=activation)
    ref.obs_encoder = nn.Identity()
    if Mf != Mi:
        ref.forward_model.sequential_net = cpu_ppo_loop.make_mlp(O + NA, O, Mf, d_fwd, out_gain=1.0,
                                                                 activation=icm_oracle.activation_module(activation))
    return ref
