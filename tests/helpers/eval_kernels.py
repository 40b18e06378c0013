"""
Kernel-level drivers for the K19 and K6 tests: an MLP actor (+ a critic for K6, with an in_dim, a width and a depth of its
own where asked) laid out in one bucket the way the kernels' layer tables expect it (per Linear: weight [out, in]
row-major padded to 4 floats, bias padded to 4 floats; log_std after the actor's layers for the Gaussian head), the
ctypes argument blocks of ppoaf_policy_step / ppoaf_policy_infer, and the same forward in float64 / float32 on the CPU.
"""
import numpy as np
import torch

HEADS = {"categorical": 0, "gaussian": 1, "multi_categorical": 2, "bernoulli": 3}
ACTS = {"relu": 0, "leaky_relu": 1, "tanh": 2}


def _pad4(n):
    return (n + 3) // 4 * 4


class Net:
    """Random MLP in_dim -> hidden^depth -> out_dim as float64 numpy layers (rounded to float32 values)."""

    def __init__(self, rng, in_dim, hidden, depth, out_dim, act, out_gain=1.0, log_std=False):
        self.in_dim, self.hidden, self.depth, self.out_dim, self.act = in_dim, hidden, depth, out_dim, act
        self.layers = []
        for l in range(depth + 1):
            i = in_dim if l == 0 else hidden
            o = out_dim if l == depth else hidden
            g = out_gain if l == depth else 1.0
            W = (rng.standard_normal((o, i)) * g / np.sqrt(i)).astype(np.float32)
            b = (rng.standard_normal(o) * 0.1 * g).astype(np.float32)
            self.layers.append((W, b))
        self.log_std = (rng.uniform(-1.5, 0.0, out_dim)).astype(np.float32) if log_std else None

    def size(self):
        n = sum(_pad4(W.size) + _pad4(b.size) for W, b in self.layers)
        return n + (_pad4(self.out_dim) if self.log_std is not None else 0)

    def flat(self):
        out = np.zeros(self.size(), np.float32)
        off = 0
        for W, b in self.layers:
            out[off:off + W.size] = W.reshape(-1); off += _pad4(W.size)
            out[off:off + b.size] = b; off += _pad4(b.size)
        if self.log_std is not None:
            out[off:off + self.out_dim] = self.log_std
        return out

    def desc(self, _lib, offset):
        d = _lib.MlpDesc(in_dim=self.in_dim, hidden=self.hidden, depth=self.depth, out_dim=self.out_dim,
                         activation=ACTS[self.act], offset=offset, size=self.size(), log_std_offset=-1)
        if self.log_std is not None:
            d.log_std_offset = self.size() - _pad4(self.out_dim)
        return d

    def forward(self, x, dtype=np.float64):
        h = np.asarray(x, dtype=dtype)
        for l, (W, b) in enumerate(self.layers):
            h = h @ W.astype(dtype).T + b.astype(dtype)
            if l < self.depth:
                h = {"relu": lambda z: np.maximum(z, 0), "leaky_relu": lambda z: np.where(z > 0, z, dtype(0.01) * z),
                     "tanh": np.tanh}[self.act](h)
        return h


class Policy:
    """Actor + critic in one device bucket, with the argument blocks of K6 and K19."""

    def __init__(self, seed, in_dim, hidden, depth, out_dim, head, act="relu", slices=(), bounds=None, out_gain=1.0,
                 device="cuda", critic_hidden=None, critic_in_dim=None, critic_depth=None, nets=None):
        """critic_in_dim / critic_depth: a critic with observations and a depth of its own (default: the actor's).
        nets: (actor, critic) already drawn -- the seed and the shape arguments are then unused."""
        from ppo_and_friends_amd import _lib
        self._lib = _lib
        rng = np.random.default_rng(seed)
        self.head, self.slices, self.device = head, tuple(slices), torch.device(device)
        if nets is not None:
            self.actor, self.critic = nets
        else:
            self.actor = Net(rng, in_dim, hidden, depth, out_dim, act, out_gain, log_std=head == "gaussian")
            self.critic = Net(rng, critic_in_dim or in_dim, critic_hidden or hidden, critic_depth or depth, 1, act)
        self.params = torch.from_numpy(np.concatenate([self.actor.flat(), self.critic.flat()])).to(self.device)
        self.bounds = None
        if bounds is not None:
            self.bounds = tuple(torch.tensor(np.asarray(b, np.float32), device=self.device) for b in bounds)
        self.min_std = 0.01

    def set_actor(self):
        """Re-upload the actor after its numpy layers were edited."""
        self.params[:self.actor.size()].copy_(torch.from_numpy(self.actor.flat()))

    def action_shape(self, E):
        if self.head == "categorical":
            return (E,), torch.int64
        if self.head == "multi_categorical":
            return (E, len(self.slices)), torch.int64
        return (E, self.actor.out_dim), torch.float32

    def _common(self, a, obs):
        a.params = self.params.data_ptr()
        a.obs = obs.data_ptr()
        a.E = obs.shape[0]
        a.head_kind = HEADS[self.head]
        a.min_std = self.min_std
        a.n_action_slices = len(self.slices)
        for j in range(8):
            a.action_slices[j] = self.slices[j] if j < len(self.slices) else 0
        if self.bounds is not None:
            a.act_lo, a.act_hi = self.bounds[0].data_ptr(), self.bounds[1].data_ptr()

    def step_args(self, obs, seed, offset, critic_obs=None):
        """ppoaf_policy_step's argument block, the outputs left to the caller (critic_obs None: the actor's rows)."""
        a = self._lib.PolicyStepArgs()
        a.actor, a.critic = self.actor.desc(self._lib, 0), self.critic.desc(self._lib, self.actor.size())
        self._common(a, obs)
        a.critic_obs = (obs if critic_obs is None else critic_obs).data_ptr()
        a.seed, a.offset = seed, offset
        return a

    def step_k6(self, obs, seed, offset, full=False, critic_obs=None):
        """ppoaf_policy_step -> action_out; full: (raw_action_out, action_out, logp_out, value_out)."""
        from ppo_and_friends_amd import kernels as K
        E = obs.shape[0]
        a = self.step_args(obs, seed, offset, critic_obs)
        shape, dt = self.action_shape(E)
        raw, act = torch.zeros(shape, dtype=dt, device=self.device), torch.zeros(shape, dtype=dt, device=self.device)
        logp, val = torch.zeros(E, device=self.device), torch.zeros(E, device=self.device)
        a.raw_action_out, a.action_out, a.logp_out, a.value_out = raw.data_ptr(), act.data_ptr(), logp.data_ptr(), val.data_ptr()
        K.policy_step(a)
        return (raw, act, logp, val) if full else act

    def infer_args(self, obs, mode, seed=0, offset=0, out=None):
        E = obs.shape[0]
        a = self._lib.PolicyInferArgs()
        a.actor = self.actor.desc(self._lib, 0)
        self._common(a, obs)
        a.mode, a.seed, a.offset = mode, seed, offset
        shape, dt = self.action_shape(E)
        if out is None:
            out = torch.full(shape, -7, dtype=dt, device=self.device)
        a.action_out = out.data_ptr()
        return a, out

    def infer(self, obs, mode, seed=0, offset=0):
        from ppo_and_friends_amd import kernels as K
        a, out = self.infer_args(obs, mode, seed, offset)
        K.policy_infer(a)
        return out


def k12_bound(x64, x32):
    """The bound rule tests/test_gpu_k12_gradients.py states for K12, per element of a tensor:
    1e-5 |x64| + 1e-5 max|x64|, raised to 4 max|x32 - x64| (the same restatement in float32) where float32 itself
    cannot do better."""
    x64 = np.asarray(x64, np.float64)
    tol = 1e-5 * np.abs(x64) + 1e-5 * np.abs(x64).max()
    return np.maximum(tol, 4.0 * np.abs(np.asarray(x32, np.float64) - x64).max())
