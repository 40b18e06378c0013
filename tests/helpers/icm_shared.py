"""
The torch-CPU oracle of an agent-shared ICM (one ICM per env over the group's concatenated observations, MultiDiscrete([n] *
agents) actions: oracle/icm_oracle.ICM(nvec=...)) in the three forms tests/test_gpu_icm_shared.py runs: the default 128s, the
baselines' D 9 / M 32 behind an encoder of 128, and the identity encoder with model widths of its own (built as
tests/helpers/icm_identity.py builds the Discrete one).
"""
import torch.nn as nn

from oracle import cpu_ppo_loop, icm_oracle


def oracle_shared_icm(O, nvec, form):
    """O: the shared observation width (agents x per-agent width).  form: dict() | dict(enc=, hidden=, enc_hidden=) |
    dict(identity=True, Mi=, Mf=[, d_inv=, d_fwd=, activation=])."""
    A = sum(nvec)
    if not form.get("identity"):
        return icm_oracle.ICM(O, A, discrete=True, nvec=nvec, **form)
    Mi, Mf = form["Mi"], form["Mf"]
    d_inv, d_fwd, act = form.get("d_inv", 2), form.get("d_fwd", 2), form.get("activation", "relu")
    ref = icm_oracle.ICM(O, A, discrete=True, nvec=nvec, enc=O, hidden=Mi, inv_depth=d_inv, fwd_depth=d_fwd, activation=act)
    ref.obs_encoder = nn.Identity()
    if Mf != Mi:
        ref.forward_model.sequential_net = cpu_ppo_loop.make_mlp(O + A, O, Mf, d_fwd, out_gain=1.0,
                                                                 activation=icm_oracle.activation_module(act))
    return ref
