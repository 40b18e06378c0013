"""
-m gpu: K18's two-layer kernels (csrc/lstm_stacked.hip) through LSTMNetwork(num_lstm_layers=2, use_hip) against the same
network in float64 on the CPU -- plain nn.LSTM(I, H, 2), nn.LayerNorm and Linear layers holding the GPU network's
parameters.  Per case: the bucket is overwritten from a seed (non-zero biases, affine LayerNorm, weights on one scale),
x [N, S, I], non-zero initial (h, c) of both layers and d out are random; compared are out, h_n and c_n of both layers and
the gradient of every parameter tensor by itself.  Bound per tensor: |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|, raised to
4 max|x32 - x64| (the same reference in float32 on the CPU) where float32 itself cannot do better (ko.deviations); no
element is left out.  Every case also checks: the no-stash forward gives the stash forward's outputs bitwise, a second
backward into the non-zero gradient bucket adds, and the [N, 2, H] state layout gives bitwise the [2, N, H] results.

Cases: H 32 / 64 / 128 (resident and streamed weights; 4, 8, 16 waves), S 1 (fill and drain only) / 2 / 5 / 16,
N 1 / 16 / 17 / 33 (tile edge, dead rows), I 1 / 17 / 256, head depth 1 / 2, F 16 / 128, out 1 / 8, the three activations.

worst deviation / bound per case (one run on the MI355X)
  H128 S1 N1 I17 d2 F16 O8 tanh      0.035  weight_ih_l1
  H128 S1 N17 I256 d1 F128 O1 relu   0.109  hn
  H128 S16 N17 I17 d2 F16 O1 relu    0.079  out
  H128 S16 N33 I256 d1 F128 O8 tanh  0.112  bias_hh_l0
  H128 S2 N16 I17 d2 F128 O1 leaky_relu 0.083  ln_w
  H128 S2 N33 I1 d1 F16 O8 tanh      0.047  bias_hh_l0
  H128 S5 N1 I256 d2 F128 O8 leaky_relu 0.051  weight_hh_l0
  H128 S5 N16 I1 d1 F16 O1 relu      0.159  ff1.bias
  H32 S1 N1 I1 d1 F16 O1 relu        0.020  weight_ih_l1
  H32 S1 N17 I17 d2 F128 O8 tanh     0.045  weight_ih_l0
  H32 S16 N17 I1 d1 F128 O8 relu     0.036  weight_ih_l0
  H32 S16 N33 I256 d2 F128 O1 leaky_relu 0.069  ff2.weight
  H32 S2 N16 I256 d1 F16 O8 leaky_relu 0.054  hn
  H32 S5 N33 I17 d2 F16 O1 tanh      0.030  ln_w
  H64 S1 N16 I256 d2 F16 O8 leaky_relu 0.047  bias_ih_l0
  H64 S1 N33 I1 d1 F128 O1 tanh      0.043  bias_ih_l1
  H64 S16 N16 I17 d1 F16 O1 tanh     0.056  out
  H64 S16 N33 I1 d2 F16 O8 leaky_relu 0.039  weight_ih_l0
  H64 S2 N1 I17 d2 F128 O1 relu      0.041  weight_hh_l0
  H64 S5 N17 I256 d1 F128 O8 relu    0.038  bias_hh_l0
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import k12_oracle as ko

pytestmark = pytest.mark.gpu

ACTS = {"relu": nn.ReLU, "leaky_relu": nn.LeakyReLU, "tanh": nn.Tanh}

#        H    S   N   I    depth F    out act
CASES = [(32, 1, 1, 1, 1, 16, 1, "relu"),
         (32, 1, 17, 17, 2, 128, 8, "tanh"),
         (32, 2, 16, 256, 1, 16, 8, "leaky_relu"),
         (32, 5, 33, 17, 2, 16, 1, "tanh"),
         (32, 16, 17, 1, 1, 128, 8, "relu"),
         (32, 16, 33, 256, 2, 128, 1, "leaky_relu"),
         (64, 1, 16, 256, 2, 16, 8, "leaky_relu"),
         (64, 1, 33, 1, 1, 128, 1, "tanh"),
         (64, 2, 1, 17, 2, 128, 1, "relu"),
         (64, 5, 17, 256, 1, 128, 8, "relu"),
         (64, 16, 16, 17, 1, 16, 1, "tanh"),
         (64, 16, 33, 1, 2, 16, 8, "leaky_relu"),
         (128, 1, 17, 256, 1, 128, 1, "relu"),
         (128, 1, 1, 17, 2, 16, 8, "tanh"),
         (128, 2, 33, 1, 1, 16, 8, "tanh"),
         (128, 2, 16, 17, 2, 128, 1, "leaky_relu"),
         (128, 5, 1, 256, 2, 128, 8, "leaky_relu"),
         (128, 5, 16, 1, 1, 16, 1, "relu"),
         (128, 16, 17, 17, 2, 16, 1, "relu"),
         (128, 16, 33, 256, 1, 128, 8, "tanh")]


def _reference(values, dims, I, H, act, x, h0, c0, dout, dtype):
    """out, h_n, c_n and every parameter gradient of the plain torch network in `dtype`, as one flat float64 vector."""
    mods = [m.to(dtype) for m in [nn.LSTM(I, H, 2), nn.LayerNorm(H)] + [nn.Linear(i, o) for i, o in dims]]
    lstm, ln, lins = mods[0], mods[1], mods[2:]
    params = [p for m in mods for p in m.parameters()]
    with torch.no_grad():
        for p, v in zip(params, values):
            p.copy_(v)
    y, (hn, cn) = lstm(x.to(dtype).transpose(0, 1), (h0.to(dtype), c0.to(dtype)))
    z = act(ln(hn[-1]))
    for lin in lins[:-1]:
        z = act(lin(z))
    out = lins[-1](z)
    out.backward(dout.to(dtype))
    return np.concatenate([t.detach().double().reshape(-1).numpy() for t in [out, hn, cn] + [p.grad for p in params]])


@pytest.mark.parametrize("H,S,N,I,depth,F,O,act", CASES)
def test_two_layer_network_against_float64(H, S, N, I, depth, F, O, act):
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    dev = torch.device("cuda", 0)
    name = f"H{H} S{S} N{N} I{I} d{depth} F{F} O{O} {act}"
    g = torch.Generator().manual_seed(1000 * H + 100 * S + N + I)
    rand = lambda *shape: torch.rand(*shape, generator=g) * 2.0 - 1.0
    net = LSTMNetwork(I, O, sequence_length=S, activation=ACTS[act](), lstm_hidden_size=H, num_lstm_layers=2,
                      ff_hidden_size=F, ff_hidden_depth=depth, name="net")
    net.flatten_parameters_(dev)
    net.use_hip = True
    assert net._hip_scope(max_layers=2) == "" and net.hip_unsupported_reason() == "2 LSTM layers (K18 covers one)"
    with torch.no_grad():
        net.flat_params.copy_(0.3 * rand(net.flat_params.numel()))
        net.layer_norm.weight.add_(1.0)
    params = net._hip_params()
    values = [p.detach().cpu() for p in params]
    x, h0, c0, dout = rand(N, S, I), 0.8 * rand(2, N, H), 1.5 * rand(2, N, H), rand(N, O)
    dims = net.ff_layers.layer_dims()
    r64 = _reference(values, dims, I, H, ACTS[act](), x, h0, c0, dout, torch.float64)
    r32 = _reference(values, dims, I, H, ACTS[act](), x, h0, c0, dout, torch.float32)
    names = ["out", "hn", "cn"] + [n for n, _ in net.lstm.named_parameters()] + ["ln_w", "ln_b"] + \
            [f"ff{i // 2}.{'weight' if i % 2 == 0 else 'bias'}" for i in range(2 * len(dims))]
    shapes = [(N, O), (2, N, H), (2, N, H)] + [tuple(p.shape) for p in params]
    offs = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])])
    tables = [("", n, int(o), s) for n, o, s in zip(names, offs, shapes)]

    def run(states, backward=True):
        net.hidden_state = tuple(s.to(dev) for s in states)
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
    out, (hn, cn) = run((h0, c0))
    g1 = grads()
    got = np.concatenate([t.double().reshape(-1).cpu().numpy() for t in [out, hn, cn] + g1])
    devs = ko.deviations(got, r64, r32, tables)
    worst = max(devs, key=lambda d: d[1])
    print(f"{name}: worst deviation / bound {worst[1]:.3f} ({worst[0]})")
    bad = ko.failures(got, r64, r32, tables)
    assert not bad, f"{name}: " + "; ".join(bad[:6])
    assert int((net.flat_grads != 0).sum()) == sum(int((t != 0).sum()) for t in g1), "padding of the gradient bucket written"
    # the no-stash (inference) forward: bitwise the training forward's outputs
    out_i, (hn_i, cn_i) = run((h0, c0), backward=False)
    assert torch.equal(out_i, out) and torch.equal(hn_i, hn) and torch.equal(cn_i, cn)
    # a second backward into the non-zero bucket adds
    run((h0, c0))
    for a, b in zip(g1, grads()):
        assert torch.equal(b, a + a)
    # the rollout buffer's [N, 2, H] rows as the state (a transposed view, as PPOPolicy.load_hidden_states leaves it)
    net.flat_grads.zero_()
    rows = tuple(s.to(dev).transpose(0, 1).contiguous().transpose(0, 1) for s in (h0, c0))
    out_r, (hn_r, cn_r) = run(rows)
    assert N == 1 or not hn_r.is_contiguous()
    assert torch.equal(out_r, out) and torch.equal(hn_r, hn) and torch.equal(cn_r, cn)
    for a, b in zip(g1, grads()):
        assert torch.equal(a, b)
