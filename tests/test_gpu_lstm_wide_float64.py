"""
-m gpu: K18's 256-wide kernels (csrc/lstm_wide.hip) through LSTMNetwork(lstm_hidden_size=256, use_hip) against the same
network in float64 on the CPU -- plain nn.LSTM(I, 256), nn.LayerNorm and Linear layers holding the GPU network's
parameters.  Per case: the bucket is overwritten from a seed (non-zero biases, affine LayerNorm, weights on one scale),
x [N, S, I], a non-zero initial (h, c) and d out are random; compared are out, h_n, c_n and the gradient of every
parameter tensor by itself.  Bound per tensor: |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|, raised to 4 max|x32 - x64| (the
same reference in float32 on the CPU) where float32 itself cannot do better (ko.deviations); no element is left out.
Every case also checks: the no-stash forward gives the stash forward's outputs bitwise, and a second backward into the
non-zero gradient bucket adds.

Cases: S 1 (no recurrent backward step) / 2 / 5 / 16, N 1 / 32 / 33 / 65 (the 32-row tile's edges, dead rows, three
workgroups), I 1 / 17 / 256, head depth 1 / 2, F 16 (one wave of the MFMA head layer) / 128, out 1 / 8, the three activations.

worst deviation / bound per case (one run on the MI355X)
  S1 N1 I1 d1 F16 O1 relu            0.180  out
  S1 N33 I256 d2 F128 O8 tanh        0.122  weight_hh_l0
  S2 N32 I17 d1 F128 O1 leaky_relu   0.037  weight_ih_l0
  S2 N65 I1 d2 F16 O8 relu           0.033  weight_hh_l0
  S5 N1 I256 d2 F128 O8 leaky_relu   0.049  weight_hh_l0
  S5 N33 I17 d1 F16 O1 tanh          0.095  ff0.bias
  S5 N32 I1 d2 F128 O1 relu          0.036  ff2.weight
  S16 N65 I17 d2 F16 O8 tanh         0.073  weight_hh_l0
  S16 N32 I256 d1 F128 O8 relu       0.064  weight_hh_l0
  S16 N33 I1 d1 F128 O1 leaky_relu   0.073  out
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import k12_oracle as ko

pytestmark = pytest.mark.gpu

ACTS = {"relu": nn.ReLU, "leaky_relu": nn.LeakyReLU, "tanh": nn.Tanh}
H = 256

#        S   N   I    depth F    out act
CASES = [(1, 1, 1, 1, 16, 1, "relu"),
         (1, 33, 256, 2, 128, 8, "tanh"),
         (2, 32, 17, 1, 128, 1, "leaky_relu"),
         (2, 65, 1, 2, 16, 8, "relu"),
         (5, 1, 256, 2, 128, 8, "leaky_relu"),
         (5, 33, 17, 1, 16, 1, "tanh"),
         (5, 32, 1, 2, 128, 1, "relu"),
         (16, 65, 17, 2, 16, 8, "tanh"),
         (16, 32, 256, 1, 128, 8, "relu"),
         (16, 33, 1, 1, 128, 1, "leaky_relu")]


def _reference(values, dims, I, act, x, h0, c0, dout, dtype):
    """out, h_n, c_n and every parameter gradient of the plain torch network in `dtype`, as one flat float64 vector."""
    mods = [m.to(dtype) for m in [nn.LSTM(I, H), nn.LayerNorm(H)] + [nn.Linear(i, o) for i, o in dims]]
    lstm, ln, lins = mods[0], mods[1], mods[2:]
    params = [p for m in mods for p in m.parameters()]
    with torch.no_grad():
        for p, v in zip(params, values):
            p.copy_(v)
    _, (hn, cn) = lstm(x.to(dtype).transpose(0, 1), (h0.to(dtype), c0.to(dtype)))
    z = act(ln(hn[-1]))
    for lin in lins[:-1]:
        z = act(lin(z))
    out = lins[-1](z)
    out.backward(dout.to(dtype))
    return np.concatenate([t.detach().double().reshape(-1).numpy() for t in [out, hn, cn] + [p.grad for p in params]])


@pytest.mark.parametrize("S,N,I,depth,F,O,act", CASES)
def test_wide_network_against_float64(S, N, I, depth, F, O, act):
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    dev = torch.device("cuda", 0)
    name = f"S{S} N{N} I{I} d{depth} F{F} O{O} {act}"
    g = torch.Generator().manual_seed(100 * S + N + I)
    rand = lambda *shape: torch.rand(*shape, generator=g) * 2.0 - 1.0
    net = LSTMNetwork(I, O, sequence_length=S, activation=ACTS[act](), lstm_hidden_size=H, ff_hidden_size=F,
                      ff_hidden_depth=depth, name="net")
    net.flatten_parameters_(dev)
    net.use_hip = True
    assert net._hip_scope(max_layers=1, wide=True) == "" and net.hip_unsupported_reason() != ""
    with torch.no_grad():
        net.flat_params.copy_(0.2 * rand(net.flat_params.numel()))
        net.layer_norm.weight.add_(1.0)
    params = net._hip_params()
    values = [p.detach().cpu() for p in params]
    x, h0, c0, dout = rand(N, S, I), 0.8 * rand(1, N, H), 1.5 * rand(1, N, H), rand(N, O)
    dims = net.ff_layers.layer_dims()
    r64 = _reference(values, dims, I, ACTS[act](), x, h0, c0, dout, torch.float64)
    r32 = _reference(values, dims, I, ACTS[act](), x, h0, c0, dout, torch.float32)
    names = ["out", "hn", "cn"] + [n for n, _ in net.lstm.named_parameters()] + ["ln_w", "ln_b"] + \
            [f"ff{i // 2}.{'weight' if i % 2 == 0 else 'bias'}" for i in range(2 * len(dims))]
    shapes = [(N, O), (1, N, H), (1, N, H)] + [tuple(p.shape) for p in params]
    offs = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])])
    tables = [("", n, int(o), s) for n, o, s in zip(names, offs, shapes)]

    def run(backward=True):
        net.hidden_state = (h0.to(dev), c0.to(dev))
        xd = x.to(dev)
        if not backward:
            with torch.no_grad():
                return net.forward_logits(xd), net.hidden_state
        out = net.forward_logits(xd)
        out.backward(dout.to(dev))
        return out.detach(), net.hidden_state

    def grads():
        offs = [(p.data_ptr() - net.flat_params.data_ptr()) // 4 for p in params]
        return [net.flat_grads[o:o + p.numel()].clone() for o, p in zip(offs, params)]

    net.flat_grads.zero_()
    out, (hn, cn) = run()
    g1 = grads()
    got = np.concatenate([t.double().reshape(-1).cpu().numpy() for t in [out, hn, cn] + g1])
    devs = ko.deviations(got, r64, r32, tables)
    worst = max(devs, key=lambda d: d[1])
    print(f"{name}: worst deviation / bound {worst[1]:.3f} ({worst[0]})")
    bad = ko.failures(got, r64, r32, tables)
    assert not bad, f"{name}: " + "; ".join(bad[:6])
    assert int((net.flat_grads != 0).sum()) == sum(int((t != 0).sum()) for t in g1), "padding of the gradient bucket written"
    # the no-stash (inference) forward: bitwise the training forward's outputs
    out_i, (hn_i, cn_i) = run(backward=False)
    assert torch.equal(out_i, out) and torch.equal(hn_i, hn) and torch.equal(cn_i, cn)
    # a second backward into the non-zero bucket adds
    run()
    for a, b in zip(g1, grads()):
        assert torch.equal(b, a + a)
