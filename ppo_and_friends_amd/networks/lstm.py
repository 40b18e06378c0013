"""
LSTM actor / critic network -- stand-in for networks/ppo_networks/lstm.py:13-127 and the
PPOLSTMNetwork base (networks/ppo_networks/base.py:136-185) of the reference, with the same
sub-module names (lstm, layer_norm, ff_layers.sequential_net.*), hence the same state_dict keys.

The recurrent forward / backward is torch-ROCm (`nn.LSTM` -> MIOpen) by default; with `use_hip` set
(PPO(update_mode="fused")) the whole forward_logits and its gradients run on K18 (csrc/lstm.hip) instead:
one forward launch, then a dgrad (BPTT) and a weight-gradient launch that adds straight into the flat gradient
bucket.  Everything around it (rollout buffer with the per-step hidden states, window gather, losses,
optimiser) is this package's device path either way.

Semantics kept from the reference:
  * the network is STATEFUL: `hidden_state` persists between forward calls and is replaced only
    when the batch size changes (lstm.py:109-113) -- a rollout steps it once per env step, an
    update assigns it from the dataset before every mini-batch (ppo.py:2312-2319);
  * a 2-D input [B, O] is one time step for B sequences, a 3-D input [B, S, O] a window of S
    steps (lstm.py:103-107); the output is computed from the LAST layer's final hidden state ->
    LayerNorm -> activation -> feed-forward head (lstm.py:115-127).
"""
import torch
import torch.nn as nn

from .. import kernels as K
from .feed_forward import FeedForwardNetwork, PPONetwork


class _HipLstm(torch.autograd.Function):
    """
    forward_logits on K18 with a gradient.  The network's parameters are inputs only so that autograd calls backward:
    their gradients are ADDED to the network's flat gradient bucket by the weight-gradient launch and None is returned
    for them.  Observations and the initial (h, c) are data (no gradient), and the final (h, c) is not differentiable.
    """

    @staticmethod
    def forward(ctx, x, h0, c0, net, *params):
        desc = net._hip_desc(x.shape[0], x.shape[1], training=True)
        out, hn, cn = K.lstm_forward(desc, x, h0, c0, stash=True)
        ctx.net, ctx.gen, ctx.shape = net, net._hip_gen, (x.shape[0], x.shape[1])
        ctx.save_for_backward(x, h0, c0)
        ctx.mark_non_differentiable(hn, cn)
        return out, hn, cn

    @staticmethod
    def backward(ctx, dout, _dhn, _dcn):
        net = ctx.net
        if ctx.gen != net._hip_gen:
            raise RuntimeError("the LSTM network ran another training forward before this backward: the workspace its "
                               "backward reads has been overwritten")
        x, h0, c0 = ctx.saved_tensors
        if dout is not None:
            desc = net._hip_desc(*ctx.shape, training=True, reuse=True)
            K.lstm_backward(desc, x, h0, c0, dout.contiguous())
        return (None, None, None, None) + (None,) * len(net._hip_params())


class PPOLSTMNetwork(PPONetwork):
    """base.py:136-185."""

    def get_zero_hidden_state(self, batch_size, device):
        hidden = torch.zeros(self.num_lstm_layers, batch_size, self.lstm_hidden_size, dtype=torch.float32,
                             device=device)
        return hidden, torch.zeros_like(hidden)

    def reset_hidden_state(self, batch_size, device):
        self.hidden_state = self.get_zero_hidden_state(batch_size, device)


class LSTMNetwork(PPOLSTMNetwork):

    def __init__(self, in_shape, out_shape, sequence_length=10, out_init=None, activation=None,
                 lstm_hidden_size=128, num_lstm_layers=1, ff_hidden_size=128, ff_hidden_depth=1, **kw_args):
        super().__init__(in_shape=in_shape, out_shape=out_shape, **kw_args)
        self.sequence_length = int(sequence_length)
        self.activation = nn.ReLU() if activation is None else activation
        self.lstm_hidden_size = int(lstm_hidden_size)
        self.num_lstm_layers = int(num_lstm_layers)
        self.lstm = nn.LSTM(self.in_size, self.lstm_hidden_size, self.num_lstm_layers)
        for name, param in self.lstm.named_parameters():          # networks/utils.py:83-111
            if "weight" in name:
                nn.init.orthogonal_(param, 2 ** 0.5)
            elif "bias" in name:
                nn.init.constant_(param, 0.0)
        self.layer_norm = nn.LayerNorm(self.lstm_hidden_size)
        self.hidden_state = None
        self.use_hip = False              # K18 instead of nn.LSTM (set by PPO(update_mode="fused"))
        self._hip_ws = None
        self._hip_gen = 0
        ff_kw_args = dict(kw_args)
        ff_kw_args["name"] = self.name + "_lstm_ff"
        self.ff_layers = FeedForwardNetwork(in_shape=self.lstm_hidden_size, out_shape=self.out_shape,
                                            hidden_size=ff_hidden_size, hidden_depth=ff_hidden_depth,
                                            activation=self.activation, is_embedded=False, out_init=out_init,
                                            **ff_kw_args)

    def _hip_params(self):
        return [p for m in (self.lstm, self.layer_norm, self.ff_layers) for p in m.parameters()]

    def hip_unsupported_reason(self):
        """'' when K18 covers this network (shapes, activation, bucket layout), else why not."""
        from ..fused_update import _activation_code
        if self.num_lstm_layers != 1:
            return f"{self.num_lstm_layers} LSTM layers (K18 covers one)"
        if self.lstm_hidden_size not in (32, 64, 128):
            return f"LSTM hidden size {self.lstm_hidden_size} is not one of 32, 64, 128"
        if self.sequence_length > 16:
            return f"sequence length {self.sequence_length} > 16"
        if self.in_size > 256:
            return f"input width {self.in_size} > 256"
        if self.out_size > 8:
            return f"output width {self.out_size} > 8"
        act = _activation_code(self.activation)
        if act is None:
            return f"activation {self.activation} is not one of ReLU / LeakyReLU(0.01) / Tanh"
        dims = self.ff_layers.layer_dims()
        F = dims[0][1]
        if len(dims) not in (2, 3) or any(d != (F, F) for d in dims[1:-1]) or dims[-1] != (F, self.out_size):
            return "the feed-forward head must have 1 or 2 hidden layers of one width"
        if F not in (16, 32, 64, 128):
            return f"feed-forward width {F} is not one of 16, 32, 64, 128"
        if self.flat_params is not None:
            off = 0
            for p in self._hip_params():
                if (p.data_ptr() - self.flat_params.data_ptr()) // 4 != off:
                    return "parameter layout differs from the kernel's"
                off += (p.numel() + 3) // 4 * 4
        return ""

    def _hip_desc(self, rows, steps, training, reuse=False):
        from ..fused_update import _activation_code
        dims = self.ff_layers.layer_dims()
        args = (self.in_size, self.lstm_hidden_size, dims[0][1], len(dims) - 1, self.out_size,
                _activation_code(self.activation), rows, steps, self.flat_params)
        if not training:
            return K.lstm_desc(*args)
        if not reuse:
            need, _ = K.lstm_sizes(K.lstm_desc(*args))
            if self._hip_ws is None or self._hip_ws.numel() < need or self._hip_ws.device != self.flat_params.device:
                self._hip_ws = torch.empty(need, dtype=torch.float32, device=self.flat_params.device)
            self._hip_gen += 1
        return K.lstm_desc(*args, grads=self.flat_grads, workspace=self._hip_ws)

    def _hip_forward_logits(self, _input):
        x = _input.unsqueeze(1) if _input.dim() == 2 else _input
        x = x.reshape(x.shape[0], x.shape[1], -1).to(torch.float32).contiguous()      # [batch, steps, in] (batch-first)
        batch_size, H = x.shape[0], self.lstm_hidden_size
        if self.hidden_state is None or self.hidden_state[0].shape[1] != batch_size:
            self.reset_hidden_state(batch_size, x.device)
        h0, c0 = (t.reshape(batch_size, H).contiguous() for t in self.hidden_state)
        params = self._hip_params()
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            out, hn, cn = _HipLstm.apply(x, h0, c0, self, *params)
        else:
            out, hn, cn = K.lstm_forward(self._hip_desc(batch_size, x.shape[1], training=False), x, h0, c0, stash=False)
        self.hidden_state = (hn.view(1, batch_size, H), cn.view(1, batch_size, H))
        return out

    def forward_logits(self, _input):
        """Everything before output_func (what the HIP distribution kernels consume)."""
        if self.use_hip:
            return self._hip_forward_logits(_input)
        out = _input.unsqueeze(0) if _input.dim() == 2 else torch.transpose(_input, 0, 1)
        batch_size = out.shape[1]
        if self.hidden_state is None or self.hidden_state[0].shape[1] != batch_size:
            self.reset_hidden_state(batch_size, out.device)
        h, c = self.hidden_state
        _, self.hidden_state = self.lstm(out.contiguous(), (h.contiguous(), c.contiguous()))
        out = self.hidden_state[0][-1]
        out = self.activation(self.layer_norm(out))
        return self.ff_layers.forward_logits(out)

    def forward(self, _input):
        return self._shape_output(self.output_func(self.forward_logits(_input)))
