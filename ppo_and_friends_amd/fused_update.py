"""
Host drivers of the fused mini-batch update kernels: K12 (MLP policies, csrc/ppo_update.hip), K14 (ICM,
csrc/icm_update.hip, csrc/icm_update_shapes.hip), K15 (MAT policies, csrc/mat_update.hip) and K22 (LSTM policies,
csrc/lstm_update.hip).  All of them run one epoch protocol (FusedEpoch):
  begin_epoch : the epoch's inputs gathered in shuffled order (one launch), the driver's own records (value-normaliser
                records of every mini-batch: one launch, one all-gather across ranks), cursor / totals reset
  run_epoch   : per mini-batch  fwd_bwd -> reduce -> [all-reduce] -> adam;
                on a single rank, `graph_chunk` consecutive mini-batches are
                captured once into a hipGraph (all launches reading the device cursor) and replayed
  end_epoch   : a launch whose bounded in-kernel wait ran out is detected and its epoch redone without that form;
                then normaliser state back to its owner, totals to the host (the only
                host read of the epoch: the KL early stop needs it)
"""
import ctypes as C
import os
import sys
from typing import Callable, NamedTuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import kernels as K
from .networks.distributions import (BernoulliDistribution, CategoricalDistribution, GaussianDistribution,
                                     MultiCategoricalDistribution)
from .networks.feed_forward import FeedForwardNetwork
from .utils import mpi_utils, peer_exchange


def _activation_code(act):
    if isinstance(act, nn.ReLU):
        return K.ACT_RELU
    if isinstance(act, nn.LeakyReLU) and abs(act.negative_slope - 0.01) < 1e-12:
        return K.ACT_LEAKY_RELU
    if isinstance(act, nn.Tanh):
        return K.ACT_TANH
    return None


class FusedOptIns(NamedTuple):
    """
    The opt-ins of a policy to the fused path, as one immutable value: field `x` is the policy's attribute `fused_x`
    (PPOPolicy's class attributes and their comments say what each switches on; PPO sets `fused_action_heads` and
    `fused_wide_critic` under update_mode="fused", the others are set by hand).  Every scope question takes one, so a
    hypothetical ("would this policy be taken with fused_wide_heads on?") is `opt._replace(...)`, never a write to the policy.
    """
    action_heads: bool = False         # MultiDiscrete / MultiBinary heads on K6 / K12
    wide_critic: bool = False          # a 512-wide critic beside a 256-wide actor (WIDE_WIDTH_PAIRS)
    wide_inputs: bool = False          # the wide pair with 65 .. 128 inputs per network (implied by wide_shapes: of())
    wide_shapes: bool = False          # the wide pair with in_dim <= 512 per network and batch sizes <= 1024
    wide_heads: bool = False           # the wide pair's actor with a head of 9 .. WIDE_HEAD_MAX outputs
    wide_ranks: bool = False           # the wide pair on N > 1 ranks
    shared_icm: bool = False           # the agent-shared ICM of an agent-grouped policy on K14
    wide_icm_actions: bool = False     # ICM Discrete / Box actions of 9 .. WIDE_HEAD_MAX classes or dimensions

    @classmethod
    def of(cls, pol):
        """The policy's opt-ins as they are now: a policy without an attribute (MAT, test doubles) has it off."""
        on = {f: bool(getattr(pol, "fused_" + f, False)) for f in cls._fields}
        on["wide_inputs"] |= on["wide_shapes"]
        return cls(**on)

    @property
    def wide_bits(self):
        """The option bits of ppoaf_ppo_update_args_t.row_pairs a wide pair sets."""
        return _lib.SPLIT_WIDE_SHAPES if self.wide_shapes else _lib.SPLIT_WIDE_INPUTS if self.wide_inputs else 0

    def actor_out_limit(self, head):
        """The widest actor output layer `_describe` takes: WIDE_HEAD_MAX for a Categorical or Gaussian head with
        `wide_heads` and `wide_critic` (that the pair is the wide one is checked where both networks are known:
        wide_head_reason), else 8."""
        ok = self.wide_heads and self.wide_critic and head in (K.HEAD_CATEGORICAL, K.HEAD_GAUSSIAN)
        return WIDE_HEAD_MAX if ok else 8


def action_head(pol, opt=None):
    """
    (head kind, slice table, '') of the policy's action distribution on K6 / K12, or (None, None, why not).  The
    MultiDiscrete and MultiBinary heads (csrc/action_heads.hpp) are taken only for a policy built with
    update_mode="fused" (PPO sets pol.fused_action_heads: opt.action_heads); "auto" keeps the torch-ROCm path for them.
    """
    dist = pol.actor.distribution
    if isinstance(dist, CategoricalDistribution):
        return K.HEAD_CATEGORICAL, (), ""
    if isinstance(dist, GaussianDistribution):
        return K.HEAD_GAUSSIAN, (), ""
    if not isinstance(dist, (MultiCategoricalDistribution, BernoulliDistribution)):
        return None, None, "unknown action distribution"
    if not (opt or FusedOptIns.of(pol)).action_heads:
        return None, None, "MultiDiscrete / MultiBinary heads run on the fused kernels under update_mode='fused' only"
    if isinstance(dist, BernoulliDistribution):
        n = int(pol.action_pred_size)
        if not 1 <= n <= 8:
            return None, None, f"MultiBinary({n}): the fused Bernoulli head covers 1 .. 8 bits"
        return K.HEAD_BERNOULLI, (), ""
    nvec = tuple(int(k) for k in dist.nvec)
    if not (1 <= len(nvec) <= 8 and min(nvec) >= 1 and sum(nvec) <= 8):
        return None, None, (f"MultiDiscrete({list(nvec)}): the fused multi-categorical head covers 1 .. 8 slices of at "
                            "least one class each, 8 classes in all")
    return K.HEAD_MULTI_CATEGORICAL, nvec, ""


def set_action_slices(args, slices):
    """The multi-categorical head's slice table into K6's / K12's args (empty for the other heads)."""
    args.n_action_slices = len(slices)
    for j in range(8):
        args.action_slices[j] = slices[j] if j < len(slices) else 0


def _describe(net, bucket, with_log_std, wide=False, max_out=8):
    """MlpDesc of a FeedForwardNetwork living in `bucket`, or (None, reason).  wide: a 512-wide network is described too
    (the critic of a policy with `fused_wide_critic`: WIDE_WIDTH_PAIRS).  max_out: the widest output layer taken (8, or
    WIDE_HEAD_MAX for the actor of a policy with `fused_wide_heads`: FusedOptIns.actor_out_limit).  Called by describe_policy
    alone: every consumer of a policy's descriptors takes them from there."""
    if not isinstance(net, FeedForwardNetwork) or net.is_embedded:
        return None, "network is not a plain FeedForwardNetwork"
    dims = net.layer_dims()
    if len(dims) < 2:
        return None, "needs at least one hidden layer"
    H = dims[0][1]
    if any(o != H for (_, o) in dims[:-1]) or any(i != H for (i, _) in dims[1:]):
        return None, "hidden layers must share one width"
    if H not in (32, 64, 128, 256) and not (wide and H == 512):
        return None, f"hidden width {H} is not one of the instantiated widths (32, 64, 128, 256)"
    act = _activation_code(net.activation)
    if act is None:
        return None, f"activation {net.activation} is not one of ReLU / LeakyReLU(0.01) / Tanh"
    out_dim = dims[-1][1]
    if out_dim > max_out:
        return None, f"output width {out_dim} > {max_out}"
    d = _lib.MlpDesc()
    d.in_dim, d.hidden, d.depth, d.out_dim, d.activation = dims[0][0], H, len(dims) - 1, out_dim, act
    base = bucket.data_ptr()
    d.offset = (net.flat_params.data_ptr() - base) // 4
    d.size = net.flat_params.numel()
    # the kernel assumes module order weight, bias per Linear, each padded to 4 floats
    off = 0
    lin = [m for m in net.sequential_net.modules() if isinstance(m, nn.Linear)]
    for m in lin:
        for p in (m.weight, m.bias):
            if (p.data_ptr() - net.flat_params.data_ptr()) // 4 != off:
                return None, "parameter layout differs from the kernel's layer table"
            off += (p.numel() + 3) // 4 * 4
    d.log_std_offset = -1
    if with_log_std:
        ls = net.distribution.log_std
        if (ls.data_ptr() - net.flat_params.data_ptr()) // 4 != off:
            return None, "log_std is not placed after the MLP parameters"
        d.log_std_offset = off
        off += (ls.numel() + 3) // 4 * 4
    if off != d.size:
        return None, "network holds parameters the fused kernel does not know about"
    return d, ""


def _reduce_totals(upd, totals):
    """
    End of an epoch: the loss totals summed over ranks -- and, in the same all-reduce, whether any rank's peer
    exchange or bounded in-kernel wait ran out of time during the epoch.  If one did, the gradients of that step were
    garbage on that rank: every rank then restores rank 0's state and continues on the RCCL path (PPO._heal_replicas),
    instead of training on with diverged replicas, stopping the job or leaving the other ranks in this all-reduce.
    """
    t = totals.clone()
    if not upd.multi:
        return t.cpu().numpy()
    broken = 0.0
    for x in (upd.xchg, getattr(upd, "xchg_sp", None)):
        if x is not None and x.status()[1] != 0:
            broken = 1.0
    if upd._bounded_wait_failure():
        broken = 1.0               # a bounded in-kernel wait of this rank ran out: its peers' exchanges timed out on it
    t = torch.cat([t, torch.tensor([broken], dtype=t.dtype, device=t.device)])
    mpi_utils.allreduce_sum_(t)
    out = t.cpu().numpy()
    if out[-1] > 0:
        upd.ppo._heal_replicas("a peer exchange wait ran out of time")
    return out[:-1]


def _switch(name, default, values=("0", "1")):
    """A PPOAF_* switch of the fused drivers; a value outside `values` is an error, not a silent default."""
    v = os.environ.get(name, default)
    if v not in values:
        raise ValueError(f"{name}={v!r}: expected {', '.join(values[:-1])} or {values[-1]}")
    return v


def split_wgrad_mode():
    """PPOAF_SPLIT_WGRAD = auto | 0 | 1: the split-wgrad chain of K12, K14 and K15 against their slab forms."""
    return _switch("PPOAF_SPLIT_WGRAD", "auto", ("auto", "0", "1"))


def rccl_comm(dev):
    """
    The communicator of the C-level fallback loops (`ppoaf_{ppo,icm,mat}_update_chain_allreduce`): a second RCCL
    communicator owned by libppoaf_hip.so, created once per process with the id travelling over torch.distributed.
    None -- on EVERY rank -- when the backend is not RCCL, FusedPolicyUpdate.rccl_loop = "python" asks for the Python loop, or any
    rank cannot bind librccl: that is voted on BEFORE the collective init (ncclCommInitRank blocks until every rank
    has called it, so no rank may enter it alone); a second vote covers an init that returned an error.
    """
    import atexit
    import torch.distributed as dist
    cls = FusedPolicyUpdate            # (the cache and the knob stay where bench.py and the tests read / set them)
    if cls._rccl_comm_cache != "unset":
        return cls._rccl_comm_cache
    comm = None
    lib = _lib.load()
    if dist.get_backend() == "nccl" and cls.rccl_loop == "c":
        rank, world = mpi_utils.get_rank(), mpi_utils.get_num_procs()

        def vote(ok):
            v = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(v, op=dist.ReduceOp.MIN)
            return int(v.item()) == 1

        buf = (C.c_char * 128)()
        if vote(lib.ppoaf_comm_unique_id(buf) == 0):                     # every rank can bind librccl (the id call is local)
            msg = torch.zeros(128, dtype=torch.uint8)
            if rank == 0:
                msg[:] = torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8)
            msg = msg.to(dev)
            dist.broadcast(msg, src=0)                                   # rank 0's id is the communicator's
            h = C.c_void_p()
            if lib.ppoaf_comm_init(rank, world, bytes(msg.cpu().numpy().tobytes()), C.byref(h)) == 0:
                comm = h
            if not vote(comm is not None):
                if comm is not None:
                    lib.ppoaf_comm_destroy(comm)
                comm = None
        if comm is not None:
            atexit.register(_destroy_rccl_comm)
    cls._rccl_comm_cache = comm
    return comm


def _destroy_rccl_comm():
    cls = FusedPolicyUpdate
    comm, cls._rccl_comm_cache = cls._rccl_comm_cache, None
    if comm not in ("unset", None):
        try:
            torch.cuda.synchronize()
            _lib.load().ppoaf_comm_destroy(comm)
        except Exception:                                                # interpreter shutdown: nothing left to release into
            pass


class BoundedWait(NamedTuple):
    """A launch form whose workgroups wait for each other in the kernel with a time bound; a wait that ran out leaves a
    non-zero error word (another process on the GPU kept a workgroup from being resident)."""
    on: Callable          # driver -> True while the driver's launches take this form
    used: str             # driver attribute set when a launch of the epoch took it
    word: Callable        # driver -> the int32 error word (a one-element view)
    disabled: str         # driver attribute holding why the form was switched off ...
    reason: str           # ... after a failure: this
    failure: str          # what a failed launch reports
    region: Callable      # driver -> the records tagged with the cursor (zeroed when it restarts), or None


class FusedEpoch:
    """
    The epoch protocol shared by the fused drivers.  A subclass supplies its launches (`_one`, optionally `_chunk`), its
    arguments (`_make_args`) and what is baked into them (`_signature`), its per-epoch inputs (`_epoch_inputs`), the
    state an epoch changes (`_epoch_state`), its RCCL fallback launch (`_chain_allreduce`) and its bounded-wait forms
    (`_waits`).
    """

    graph_chunk = 32
    n_totals = 9                       # length of the device totals
    min_tail_rows = 2                  # a smaller tail mini-batch is not launched
    _waits = ()

    # ---- fused tail launches (K12, K15): weight gradients + clip norms + Adam in one launch whose workgroups wait for each other
    tail_wait_seconds = 2.0            # bound of the in-kernel wait for the other workgroups' norm records
    tail_launches = 0                  # launches issued in this process (tests: the path really ran; graph replays not counted)

    def __init__(self, ppo, policy_id):
        self.ppo, self.policy_id = ppo, policy_id
        pol = self.pol = ppo.policies[policy_id]
        self.world = mpi_utils.get_num_procs()
        self.multi = mpi_utils.distributed_path()       # collectives + eager launches (N > 1, or its rehearsal)
        self.B = ppo.batch_size
        self.cursor = torch.zeros(1, dtype=torch.int64, device=pol.device)
        self.totals = torch.zeros(self.n_totals, dtype=torch.float64, device=pol.device)
        self._lib = _lib.load()
        self.perm = self.tables = self._split_space = self._tail_ctl = self._epoch_snapshot = None
        self._graphs, self._args = {}, {}
        self.n_full = self.tail = self.n_done = 0

    def _open_exchange(self, floats):
        """N > 1: the per-mini-batch gradient exchange.  K17 over peer mappings when every rank can (same host, IPC +
        self-test passed: collective decision), else the RCCL all-reduce in an eager loop."""
        self.xchg, self.xchg_reason = (peer_exchange.open_exchange(floats, self.pol.device) if self.multi
                                       else (None, "single rank"))

    def drop_peer_exchange(self, why):
        """PPO._heal_replicas (collective, every rank): peer exchanges closed, the RCCL all-reduce path from here on."""
        for name in ("xchg", "xchg_sp"):
            x = getattr(self, name, None)
            if x is not None:
                x.close()
                setattr(self, name, None)
                self.xchg_reason = f"disabled: {why}"
        self._graphs.clear()
        self._args = {}

    # ------------------------------------------------------------------ args
    def _args_for(self, B):
        if B not in self._args:
            self._args[B] = self._make_args(B)
        return self._args[B]

    def _tail_ctl_ptr(self, args):
        """Control block of the fused tail launch (size from the driver's `_tail_ctl_bytes` entry point)."""
        if self._tail_ctl is None:
            need = C.c_int64(0)
            _lib.check(getattr(self._lib, "ppoaf_" + self._tail_ctl_bytes)(C.byref(args), C.byref(need)), self._tail_ctl_bytes)
            # zeroed once, then kept: the block carries the launch tag from one launch to the next
            self._tail_ctl = torch.zeros((int(need.value) + 63) // 64 * 16, dtype=torch.int32, device=self.pol.device)
        FusedEpoch.tail_launches += 1
        return self._tail_ctl.data_ptr()

    # ----------------------------------------------------------------- epoch
    def begin_epoch(self, perm):
        N = perm.numel()
        if self.perm is None or self.perm.numel() != N:
            self.perm = torch.empty(N, dtype=torch.int64, device=self.pol.device)
            self._graphs.clear()
        self.perm.copy_(perm)
        self._epoch_inputs(N)
        self._restart_epoch()
        sig = self._signature()
        if self._args.get("sig") != sig:
            self._args = {"sig": sig}
            self._graphs.clear()
        self.n_full, self.tail = N // self.B, N % self.B

    def _epoch_tables(self, attr, N, shapes):
        """The epoch's tables kept in `self.<attr>`: {name: (row shape, dtype, device)} -> tensors of N rows each, allocated
        anew (captured graphs and args dropped: they hold the addresses) only when N changes."""
        t = getattr(self, attr, None)
        if t is None or next(iter(t.values())).shape[0] != N:
            t = {k: torch.empty((N,) + tuple(shape), dtype=dtype, device=device) for k, (shape, dtype, device) in shapes.items()}
            setattr(self, attr, t)
            self._graphs.clear()
            self._args = {}
        return t

    def _gather_tables(self, fields, into="tables"):
        """K4 over the whole epoch: every input field of the update in shuffled order (one launch), into `self.<into>`."""
        buf, N = self.pol.buffer, self.perm.numel()
        flat = lambda x: x.view((buf.num_transitions,) + tuple(x.shape[2:]))
        t = self._epoch_tables(into, N, {k: (v.shape[2:], v.dtype, v.device) for k, v in fields.items()})
        K.minibatch_gather([(flat(v), t[k]) for k, v in fields.items()], self.perm, buf.row_map)
        return t

    def _restart_epoch(self):
        """The cursor starts over: totals, mini-batch count and every record region tagged with the cursor back to zero."""
        self.cursor.zero_()
        self.totals.zero_()
        self.n_done = 0
        for w in self._waits:
            r = w.region(self)
            if r is not None:
                r.zero_()

    def _chunk(self, args, n):
        for _ in range(n):
            self._one(args)

    def _c_loop(self, args, n):
        """The RCCL fallback (N > 1 without K17) issued from C, <= 256 mini-batches per call.  False when the library has no
        RCCL communicator of its own (gloo tests: collectives through the host; rccl_loop = "python")."""
        comm = None if mpi_utils._needs_staging(self.cursor) else rccl_comm(self.pol.device)
        if comm is None:
            return False
        ref, st = C.byref(args), K.stream()
        while n > 0:
            k = min(n, 256)
            self._chain_allreduce(ref, comm, k, st)
            n -= k
        return True

    def run_epoch(self):
        self._args_for(self.B)                           # (building the args may resize state the snapshot holds)
        self._epoch_snapshot = None
        if not self.multi and any(w.on(self) for w in self._waits):
            # what the epoch starts from (a few buckets of <= 1 MB: device-to-device copies), should a bounded wait run out
            self._epoch_snapshot = [t.clone() for t in self._epoch_state()]
        self._launch_epoch()

    def _launch_epoch(self):
        args = self._args_for(self.B)
        left = self.n_full
        if left > 0 and self.multi and self.xchg is None and self._c_loop(args, left):
            self.n_done += left
            left = 0
        use_graph = self.ppo.use_graphs and (not self.multi or self.xchg is not None)   # RCCL calls are not captured
        chunk = self.graph_chunk if self.n_full < 8 * self.graph_chunk else 4 * self.graph_chunk   # long epochs: fewer, longer graphs
        while left > 0:
            if use_graph and left >= chunk:
                g = self._graphs.get(chunk)
                if g is None:
                    s = torch.cuda.Stream()
                    s.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(s):
                        self._chunk(args, chunk)          # warm-up pass: these mini-batches are real
                    torch.cuda.current_stream().wait_stream(s)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._chunk(args, chunk)          # capture only
                    self._graphs[chunk] = g
                else:
                    g.replay()
                left -= chunk
                self.n_done += chunk
            else:
                self._one(args)
                left -= 1
                self.n_done += 1
        if self.tail >= self.min_tail_rows:
            self._one(self._args_for(self.tail))
            self.n_done += 1

    # ---- a launch whose workgroups could not all be resident must not cost the run: the epoch is redone without that form
    def _bounded_wait_failure(self):
        """After a host synchronisation: '' or which bounded in-kernel waits of the epoch's launches ran out.  Each form that
        failed is switched off (with the reason); the captured graphs and the args, which bake the forms in, are dropped."""
        why = []
        for w in self._waits:
            if not getattr(self, w.used, False):
                continue
            setattr(self, w.used, False)
            word = w.word(self)
            if int(word.item()) != 0:
                word.zero_()
                setattr(self, w.disabled, w.reason)
                why.append(w.failure)
        if why:
            self._graphs.clear()
            self._args = {"sig": self._args.get("sig")}
        return "; ".join(why)

    def _check_persistent(self):
        """Raising form (tests, probes that drive single launches)."""
        why = self._bounded_wait_failure()
        if why:
            raise _lib.PpoafError(why)

    def end_epoch(self):
        """-> numpy totals (summed over ranks).  On a single rank, an epoch in which a bounded wait ran out is redone from
        its starting state without the failed form, until an epoch comes back clean (each failure switches one more form
        off); nothing of a failed epoch reaches the normaliser or the totals."""
        if not self.multi and any(getattr(self, w.used, False) for w in self._waits):
            torch.cuda.current_stream().synchronize()
            why = self._bounded_wait_failure()
            while why:
                if self._epoch_snapshot is None:
                    raise _lib.PpoafError(why)
                print(f"[ppo_and_friends_amd] {why}; restoring the epoch's starting state and running the epoch again without it",
                      file=sys.stderr, flush=True)
                for t, keep in zip(self._epoch_state(), self._epoch_snapshot):
                    t.copy_(keep)
                self._restart_epoch()
                self._launch_epoch()
                torch.cuda.current_stream().synchronize()
                why = self._bounded_wait_failure()
        self._publish()
        return _reduce_totals(self, self.totals)         # synchronises with the device (N > 1: a failed launch is voted on there)

    def _publish(self):
        """After a clean epoch: what the driver hands back besides the totals."""


# ---- K12 and K15: the value-normaliser records and the chained mini-batches
def _init_normaliser(upd):
    dev = upd.pol.device
    upd.vn_mean = torch.zeros(2, dtype=torch.float32, device=dev)
    upd.vn_var = torch.ones(2, dtype=torch.float32, device=dev)
    upd.vn_count = torch.full((2,), 1e-4, dtype=torch.float64, device=dev)
    upd.records = upd.adv_records = None


def _seed_normaliser(upd):
    rs = upd.ppo.value_normalizers[upd.policy_id].running_stats
    upd.vn_mean[0:1].copy_(rs.mean_t); upd.vn_var[0:1].copy_(rs.var_t); upd.vn_count[0:1].copy_(rs.count_t)


def _publish_normaliser(upd):
    """The normaliser state after the epoch's last mini-batch back to its owner."""
    ppo = upd.ppo
    if ppo.normalize_values:
        rs = ppo.value_normalizers[upd.policy_id].running_stats
        slot = upd.n_done & 1
        rs.mean_t.copy_(upd.vn_mean[slot:slot + 1]); rs.var_t.copy_(upd.vn_var[slot:slot + 1])
        rs.count_t.copy_(upd.vn_count[slot:slot + 1])
        if upd.tail == 1:
            # ppo.py:2299-2306: a size-1 batch still updates the normaliser, then is skipped (quirk Q9)
            rs.integrate_records(upd.records[upd.n_full].contiguous())


def _loss_args(upd, a, B):
    """The fields of K12's and K15's args that agree: the epoch's tables, cursor, normaliser records, loss constants."""
    pol, ppo, buf, t = upd.pol, upd.ppo, upd.pol.buffer, upd.tables
    # inputs come from the per-epoch tables in shuffled order (begin_epoch): no index -> data dependent load
    a.critic_obs, a.raw_actions = t["critic_obs"].data_ptr(), t["raw_actions"].data_ptr()
    a.advantages, a.old_log_probs = t["advantages"].data_ptr(), t["log_probs"].data_ptr()
    a.rewards_to_go, a.values = t["rewards_to_go"].data_ptr(), buf.values.data_ptr()
    a.inputs_in_batch_order, a.n_rows = 1, buf.num_transitions
    a.cursor, a.B, a.batch_stride = upd.cursor.data_ptr(), B, upd.B
    a.normalize_values, a.n_ranks = int(bool(ppo.normalize_values)), upd.world
    a.normalize_adv, a.use_huber = int(bool(ppo.normalize_adv)), int(bool(pol.use_huber_loss))
    a.vn_mean, a.vn_var, a.vn_count = upd.vn_mean.data_ptr(), upd.vn_var.data_ptr(), upd.vn_count.data_ptr()
    a.vn_records = upd.records.data_ptr() if upd.records is not None else None
    a.adv_records = upd.adv_records.data_ptr() if upd.adv_records is not None else None
    a.surr_clip, a.entropy_weight = float(pol.surr_clip), float(pol.entropy_weight())
    a.kl_loss_weight, a.huber_delta = float(pol.kl_loss_weight), 10.0
    a.loss_partials, a.totals = upd.loss_partials.data_ptr(), upd.totals.data_ptr()
    a.mb_offset, a.cursor_advance = 0, 1


def _loss_signature(upd):
    """What K12 and K15 bake into captured launches besides buffer addresses."""
    pol, ppo = upd.pol, upd.ppo
    return (None if upd.records is None else upd.records.data_ptr(),
            None if upd.adv_records is None else upd.adv_records.data_ptr(),
            float(pol.entropy_weight()), float(pol.surr_clip), float(pol.kl_loss_weight),
            bool(pol.use_huber_loss), pol.gradient_clip, bool(ppo.normalize_adv), bool(ppo.normalize_values))


def _chunk_with_offsets(upd, args, n):
    """n consecutive mini-batches with their index baked in: one cursor update for the whole chain."""
    try:
        for j in range(n):
            args.mb_offset = j
            args.cursor_advance = n if j == n - 1 else 0
            upd._one(args)
    finally:
        args.mb_offset, args.cursor_advance = 0, 1


# the fused tail launch of K12 and K15 (the same control-block layout: csrc/tail_sync.hpp TailCtl)
_TAIL_WAIT = BoundedWait(
    on=lambda u: u.tail_reason() == "", used="_tail_used", word=lambda u: u._tail_ctl[2:3],      # TailCtl.error
    disabled="_tail_disabled", reason="a wait for the other workgroups' norm records ran out of time",
    failure="ppo_update_wgrad_adam: a wait ran out of time -- the launch's workgroups were not all resident at once "
            "(another process on this GPU?)",
    region=lambda u: None)             # (the block carries the launch tag from one launch to the next: never zeroed)


class FusedLstm:
    """
    Coverage of K18 (csrc/lstm.hip) for an LSTM actor / critic pair.  Such a policy is trained by PPO's mini-batch loop
    (_minibatch_step): under update_mode="fused" its two networks run forward_logits and its gradients on K18, next to
    the distribution, loss and Adam kernels that loop already uses.  (FusedPolicyUpdate.unsupported_reason stays the
    MLP-only test: it also picks the K6 rollout-step kernel, which never sees an LSTM policy.)
    """

    @staticmethod
    def unsupported_reason(pol):
        """'' when K18 covers both networks of this LSTM policy, else why not."""
        from .networks.lstm import LSTMNetwork
        if not pol.using_lstm:
            return "not an LSTM policy"
        if pol.agent_grouping:
            return "LSTM inside agent-grouped (MAT) policies is not covered"
        if not isinstance(pol.actor.distribution, (CategoricalDistribution, GaussianDistribution)):
            return "actor: only categorical and Gaussian action distributions are covered"
        for tag, net in (("actor", pol.actor), ("critic", pol.critic)):
            if not isinstance(net, LSTMNetwork):
                return f"{tag}: {type(net).__name__} is not an LSTMNetwork"
            why = net.hip_unsupported_reason()
            if why:
                return f"{tag}: {why}"
        if pol.critic.out_size != 1:
            return "critic must have one output"
        return ""


def _describe_lstm_update(pol, B):
    """_lib.LstmUpdateArgs with the shapes of an LSTM policy's two networks (no pointer set), for a mini-batch of B rows."""
    a = _lib.LstmUpdateArgs()
    for tag, net in (("actor", pol.actor), ("critic", pol.critic)):
        d = getattr(a, tag)
        dims = net.ff_layers.layer_dims()
        d.in_dim, d.hidden, d.ff_hidden, d.ff_depth = net.in_size, net.lstm_hidden_size, dims[0][1], len(dims) - 1
        d.out_dim, d.activation = net.out_size, _activation_code(net.activation)
        d.rows, d.steps = B, net.sequence_length
    a.head_kind = K.HEAD_GAUSSIAN if isinstance(pol.actor.distribution, GaussianDistribution) else K.HEAD_CATEGORICAL
    a.B = a.batch_stride = B
    return a


class FusedLstmUpdate(FusedEpoch):
    """
    Host driver of K22 (csrc/lstm_update.hip): one epoch of PPO._ppo_batch_train for an LSTM actor / critic pair, three
    launches per mini-batch (fwd_bwd -> wgrad -> adam) that read the device cursor.  The windows and the stored hidden
    states are read through `perm` / `row_map` inside fwd_bwd (windows overlap and the states change during the epoch,
    so neither can be tabled); the fields of the windows' LAST position are gathered once per epoch in shuffled order.
    The optimiser state is the policy's own (FlatAdam's tensors), so `pol.fused_lstm_update = False` -- today's
    mini-batch loop -- and checkpoints continue from the same state.
    """

    launches = 0                       # launches issued in this process (tests: the path really ran; graph replays not counted)

    @staticmethod
    def unsupported_reason(pol, batch_size):
        """'' when K22 covers this policy at this batch size, else why the mini-batch loop runs."""
        why = FusedLstm.unsupported_reason(pol)
        if why:
            return why
        ha, hc = pol.actor.lstm_hidden_size, pol.critic.lstm_hidden_size
        if ha != hc:
            return f"LSTM hidden sizes differ (actor {ha}, critic {hc}): one K22 launch has one block size"
        if pol.actor.sequence_length != pol.critic.sequence_length:
            return f"sequence lengths differ (actor {pol.actor.sequence_length}, critic {pol.critic.sequence_length})"
        if batch_size < 2:
            return "batch size < 2"
        return K.lstm_update_refusal(_describe_lstm_update(pol, batch_size))     # host only: nothing is launched

    def __init__(self, ppo, policy_id):
        super().__init__(ppo, policy_id)
        pol, dev = self.pol, self.pol.device
        self.n_wg = (self.B + K.UPDATE_ROWS_PER_WG - 1) // K.UPDATE_ROWS_PER_WG
        _init_normaliser(self)
        self.loss_partials = torch.zeros(2, self.n_wg, 8, dtype=torch.float32, device=dev)
        self.S = pol.actor.sequence_length
        self.actor_size = pol.actor.bucket_size()
        self.gauss = isinstance(pol.actor.distribution, GaussianDistribution)
        self.log_std_offset = -1
        if self.gauss:
            self.log_std_offset = (pol.actor.distribution.log_std.data_ptr() - pol.policy_params.data_ptr()) // 4
        q = _describe_lstm_update(pol, self.B)
        q.bucket_total, q.actor_size = pol.policy_params.numel(), self.actor_size
        floats, doubles, self.lds_bytes = K.lstm_update_sizes(q)
        self.workspace = torch.zeros(floats, dtype=torch.float32, device=dev)
        self.norm_scratch = torch.zeros(doubles, dtype=torch.float64, device=dev)
        self.perm_last = None
        self._open_exchange(pol.policy_params.numel())

    # ------------------------------------------------------------------ args
    def _make_args(self, B):
        pol, ppo, buf, ds, t = self.pol, self.ppo, self.pol.buffer, self.pol.dataset, self.tables
        a = _describe_lstm_update(pol, B)
        a.batch_stride = self.B
        na = self.actor_size
        a.params, a.grads = pol.policy_params.data_ptr(), pol.policy_grads.data_ptr()
        a.exp_avg, a.exp_avg_sq = pol.policy_exp_avg.data_ptr(), pol.policy_exp_avg_sq.data_ptr()
        a.actor.params, a.actor.grads = a.params, a.grads
        a.critic.params, a.critic.grads = a.params + 4 * na, a.grads + 4 * na
        a.bucket_total, a.actor_size, a.log_std_offset = pol.policy_params.numel(), na, self.log_std_offset
        a.step_counts, a.lr = pol.policy_step_counts.data_ptr(), pol.policy_lr.data_ptr()
        a.norm_scratch, a.norm_scratch_doubles = self.norm_scratch.data_ptr(), self.norm_scratch.numel()
        a.beta1, a.beta2, a.adam_eps = 0.9, 0.999, 1e-5
        a.grad_scale = 1.0 / self.world
        a.max_norm = float(pol.gradient_clip) if pol.gradient_clip is not None else 0.0
        a.obs, a.critic_obs = buf.observations.data_ptr(), buf.critic_observations.data_ptr()
        a.terminal = ds.terminal_positions.data_ptr() if self.S > 1 else None
        a.perm, a.row_map = self.perm.data_ptr(), ds.row_map.data_ptr()
        a.n_rows, a.n_items = buf.num_transitions, self.perm.numel()
        a.raw_actions, a.advantages = t["raw_actions"].data_ptr(), t["advantages"].data_ptr()
        a.old_log_probs, a.rewards_to_go = t["log_probs"].data_ptr(), t["rewards_to_go"].data_ptr()
        a.values = buf.values.data_ptr()
        h = buf.hidden
        a.actor_hidden, a.actor_cell = h["actor_hidden"].data_ptr(), h["actor_cell"].data_ptr()
        a.critic_hidden, a.critic_cell = h["critic_hidden"].data_ptr(), h["critic_cell"].data_ptr()
        a.cursor = self.cursor.data_ptr()
        a.normalize_values, a.n_ranks = int(bool(ppo.normalize_values)), self.world
        a.normalize_adv, a.use_huber = int(bool(ppo.normalize_adv)), int(bool(pol.use_huber_loss))
        a.vn_mean, a.vn_var, a.vn_count = self.vn_mean.data_ptr(), self.vn_var.data_ptr(), self.vn_count.data_ptr()
        a.vn_records = self.records.data_ptr() if self.records is not None else None
        a.adv_records = self.adv_records.data_ptr() if self.adv_records is not None else None
        a.surr_clip, a.entropy_weight = float(pol.surr_clip), float(pol.entropy_weight())
        a.kl_loss_weight, a.huber_delta = float(pol.kl_loss_weight), 10.0
        a.min_std = float(getattr(pol.actor.distribution, "min_std", 0.01))
        a.loss_partials, a.totals = self.loss_partials.data_ptr(), self.totals.data_ptr()
        a.workspace, a.workspace_floats = self.workspace.data_ptr(), self.workspace.numel()
        why = K.lstm_update_refusal(a, pointers=True)
        if why:
            raise _lib.PpoafError(why)
        return a

    def _signature(self):
        """Everything baked into captured launches; a change re-captures."""
        pol, buf, ds = self.pol, self.pol.buffer, self.pol.dataset
        return (buf.observations.data_ptr(), buf.critic_observations.data_ptr(), buf.values.data_ptr(), buf.num_transitions,
                ds.row_map.data_ptr(), ds.terminal_positions.data_ptr() if self.S > 1 else 0, self.perm.data_ptr(),
                self.perm.numel(), tuple(v.data_ptr() for v in self.tables.values()),
                tuple(v.data_ptr() for v in buf.hidden.values()), pol.policy_params.data_ptr(), float(pol.lr()),
                self.world) + _loss_signature(self)

    # ----------------------------------------------------------------- epoch
    def _epoch_inputs(self, N):
        pol, ppo = self.pol, self.ppo
        buf = pol.buffer
        if self.perm_last is None or self.perm_last.numel() != N:
            self.perm_last = torch.empty(N, dtype=torch.int64, device=pol.device)
        torch.add(self.perm, self.S - 1, out=self.perm_last)          # every non-observation field: the window's last position
        fields = dict(raw_actions=buf.raw_actions, advantages=buf.advantages, log_probs=buf.log_probs,
                      rewards_to_go=buf.rewards_to_go)
        flat = lambda x: x.view((buf.num_transitions,) + tuple(x.shape[2:]))
        t = self.tables
        if t is None or next(iter(t.values())).shape[0] != N:
            t = self.tables = {k: torch.empty((N,) + tuple(v.shape[2:]), dtype=v.dtype, device=v.device) for k, v in fields.items()}
            self._graphs.clear()
            self._args = {}
        K.minibatch_gather([(flat(v), t[k]) for k, v in fields.items()], self.perm_last, buf.row_map)
        nb = (N + self.B - 1) // self.B
        if ppo.normalize_values:
            local = K.minibatch_moments(buf.rewards_to_go.view(-1), self.perm_last, buf.row_map, self.B)
            if self.multi:
                rec = mpi_utils.allgather_records(local.reshape(-1)).view(self.world, nb, 3).permute(1, 0, 2).contiguous()
            else:
                rec = local.view(nb, 1, 3)
            if self.records is None or self.records.shape != rec.shape:
                self.records = torch.empty_like(rec)
                self._graphs.clear()
            self.records.copy_(rec)
            _seed_normaliser(self)
        if ppo.normalize_adv:
            if self.adv_records is None or self.adv_records.shape[0] != nb:
                self.adv_records = torch.empty(nb, 3, dtype=torch.float64, device=pol.device)
                self._graphs.clear()
            K.minibatch_moments(buf.advantages.view(-1), self.perm_last, buf.row_map, self.B, out=self.adv_records)

    def _epoch_state(self):
        pol = self.pol
        return [pol.policy_params, pol.policy_exp_avg, pol.policy_exp_avg_sq, pol.policy_step_counts, self.vn_mean, self.vn_var,
                self.vn_count, pol.buffer.values] + list(pol.buffer.hidden.values())

    _publish = _publish_normaliser

    def gradient_only(self, args):
        """fwd_bwd + wgrad of ONE mini-batch, no optimiser step: the gradient bucket tests compare.  (The wgrad launch
        advances the Adam step counters as usual; the cursor stays.)"""
        lib, st, ref = self._lib, K.stream(), C.byref(args)
        _lib.check(lib.ppoaf_lstm_update_fwd_bwd(ref, st), "lstm_update_fwd_bwd")
        _lib.check(lib.ppoaf_lstm_update_wgrad(ref, st), "lstm_update_wgrad")
        FusedLstmUpdate.launches += 2

    def _one(self, args):
        """One mini-batch: 3 launches; on N > 1 the gradient exchange sits between wgrad and adam (K17: one launch that
        also leaves both clip norms; else an all-reduce and a norm pass)."""
        lib, st, ref = self._lib, K.stream(), C.byref(args)
        rc = lib.ppoaf_lstm_update_fwd_bwd(ref, st) or lib.ppoaf_lstm_update_wgrad(ref, st)
        n = 3
        if rc == 0 and not self.multi:
            rc = lib.ppoaf_lstm_update_adam(ref, 0, st)
        elif rc == 0 and self.xchg is not None:
            g = self.pol.policy_grads
            self.xchg.allreduce(g, g, split_floats=self.actor_size, norm_scale=args.grad_scale, norm_out=self.norm_scratch,
                                stream=st)
            rc = lib.ppoaf_lstm_update_adam(ref, 2, st)
            n = 4
        elif rc == 0:
            mpi_utils.allreduce_sum_(self.pol.policy_grads)
            rc = lib.ppoaf_lstm_update_adam(ref, 1, st)
            n = 4
        FusedLstmUpdate.launches += n
        if rc != 0:
            _lib.check(rc, "lstm_update")

    def _c_loop(self, args, n):
        return False                   # (no C chain for this driver: the all-reduce fallback is the eager loop)


# the (actor width, critic width) pairs K6+K7 and K12 are instantiated for (csrc/ppo_update_dev.hpp: PPOAF_WIDTH_PAIRS)
WIDTH_PAIRS = ((32, 32), (64, 64), (128, 128), (256, 256), (128, 256), (64, 128), (64, 256), (32, 256), (32, 64))
# ... and the pairs with a 512-wide critic (PPOAF_WIDTH_PAIRS_WIDE; csrc/ppo_update_rowtile_wide.hpp), taken only for a policy
# whose `fused_wide_critic` is true (PPO sets it under update_mode="fused"; "auto" keeps the torch-ROCm path for them): the
# split-wgrad chain in its three-launch form, single rank, in_dim <= 64, batch sizes <= 512.  With the opt-in
# `PPOPolicy.fused_wide_inputs` in_dim <= 128: the layer-0 panel of a network with more than 64 inputs takes a row stride of
# 128 floats (the bit PPOAF_SPLIT_WIDE_INPUTS of ppoaf_ppo_update_args_t.row_pairs; csrc/ppo_update_dev.hpp: split_xld).
# With the opt-in `PPOPolicy.fused_wide_shapes` (which implies the other; PPOAF_SPLIT_WIDE_SHAPES) in_dim <= 512, as far as
# each row-tile body's LDS goes, on panels of stride 256 or 512, and batch sizes <= 1024: the weight-gradient launch then
# runs a mini-batch of more than 32 chunks of 16 rows in passes of 32 (csrc/ppo_update_split.hip).
# With the opt-in `PPOPolicy.fused_wide_ranks` N > 1 ranks: the same three launches with the gradient all-reduce between wgrad
# and Adam (Adam mode 1; from C: ppoaf_ppo_update_chain_allreduce's split form).  No K17 route: FusedPolicyUpdate.__init__.
WIDE_WIDTH_PAIRS = ((256, 512),)


# With the opt-in `PPOPolicy.fused_wide_heads` the wide pair's actor takes 9 .. WIDE_HEAD_MAX outputs under a Categorical or a
# tanh-Gaussian head (Discrete(18), Box(17)): kernels of their own for K6+K7, K12's fwd_bwd and K19 (csrc/policy_wide_heads.hip,
# csrc/ppo_update_wide_heads.hip), chosen by the library from out_dim.  Every other pair and head keeps 8.
WIDE_HEAD_MAX = 24


def wide_head_reason(a, c):
    """'' for described networks whose actor head the kernels take, else the limit: more than 8 outputs exist at the wide pair
    only."""
    if a.out_dim <= 8 or (a.hidden, c.hidden) in WIDE_WIDTH_PAIRS:
        return ""
    return (f"hidden widths (actor {a.hidden}, critic {c.hidden}): actor output width {a.out_dim} > 8 (fused_wide_heads takes "
            f"9 .. {WIDE_HEAD_MAX} outputs at the wide pair {WIDE_WIDTH_PAIRS[0]} only)")


def panel_stride(in_dim):
    """Row stride (floats) of a network's layer-0 panel in the split workspace (csrc/ppo_update_dev.hpp: split_xld)."""
    return next((s for s in (64, 128, 256) if in_dim <= s), 512)


class PolicyDesc(NamedTuple):
    """What K6+K7, K12 and K19 are told about an MLP policy (describe_policy)."""
    head: int                          # K.HEAD_*
    slices: tuple                      # the multi-categorical head's slice table (empty for the other heads)
    actor: "_lib.MlpDesc"
    critic: "_lib.MlpDesc"
    wide: bool                         # the pair is one of WIDE_WIDTH_PAIRS


def describe_policy(pol, opt=None):
    """(PolicyDesc, '') of an MLP actor / critic the fused kernels are instantiated for, under the opt-ins `opt` (None: the
    policy's own), or (None, why not).  The one description that the update's scope check and driver, the rollout step and
    the inference step take their descriptors from; what depends on the batch size, the ranks, the environment or the
    library is FusedPolicyUpdate.unsupported_reason's."""
    if opt is None:
        opt = FusedOptIns.of(pol)
    head, slices, why = action_head(pol, opt)
    if head is None:
        return None, why
    nets = []
    for name, net, log_std, wide, max_out in (("actor", pol.actor, head == K.HEAD_GAUSSIAN, False, opt.actor_out_limit(head)),
                                              ("critic", pol.critic, False, opt.wide_critic, 8)):
        d, why = _describe(net, pol.policy_params, log_std, wide, max_out)
        if d is None:
            return None, f"{name}: {why}"
        nets.append(d)
    a, c = nets
    if c.out_dim != 1:
        return None, "critic must have one output"
    if a.offset != 0 or c.offset != a.size:
        return None, "actor and critic buckets are not adjacent"
    wide = (a.hidden, c.hidden) in WIDE_WIDTH_PAIRS              # (a 512-wide critic is described for opt.wide_critic only)
    if (a.hidden, c.hidden) not in WIDTH_PAIRS and not wide:
        return None, f"hidden widths (actor {a.hidden}, critic {c.hidden}) are not an instantiated pair"
    if wide_head_reason(a, c):
        return None, wide_head_reason(a, c)
    return PolicyDesc(head, slices, a, c, wide), ""


def set_head_args(args, desc, dist):
    """The action head of a described policy into K6's / K19's args: kind, slice table, and the Gaussian head's min_std and
    action bounds (dist: the actor's distribution)."""
    args.head_kind = desc.head
    set_action_slices(args, desc.slices)
    args.min_std = float(getattr(dist, "min_std", 0.01))
    lo, hi = dist.bound_tensors() if desc.head == K.HEAD_GAUSSIAN else (None, None)
    args.act_lo = None if lo is None else lo.data_ptr()
    args.act_hi = None if hi is None else hi.data_ptr()


def _would_take(driver, pol, batch_size, flag, *also):
    """True when the opt-in `flag` is off and `driver` takes the policy with it (and the opt-ins `also`) switched on: the
    hypothetical is asked of a changed FusedOptIns, the policy is only read."""
    opt = FusedOptIns.of(pol)
    if getattr(opt, flag):
        return False
    return driver.unsupported_reason(pol, batch_size, opt._replace(**dict.fromkeys((flag,) + also, True))) == ""


def opt_in_hint(pol, batch_size, update_mode):
    """The clause `verbose` appends to a refusal of FusedPolicyUpdate: the one switch that would take the policy -- under
    "auto" update_mode="fused" itself, then with fused_wide_heads, then with fused_wide_ranks; under "fused" the latter two --
    or '' (a policy that misses two opt-ins at once gets none)."""
    F = FusedPolicyUpdate
    if update_mode == "fused":
        if F.wide_heads_would_take(pol, batch_size):
            return "; PPOPolicy.fused_wide_heads = True would take it on the fused kernels"
        if F.wide_ranks_would_take(pol, batch_size):
            return "; PPOPolicy.fused_wide_ranks = True would take it on the fused kernels"
        return ""
    if F.fused_mode_would_take(pol, batch_size):
        return "; update_mode='fused' would take it on the fused kernels"
    if F.wide_heads_would_take(pol, batch_size):
        return "; update_mode='fused' with PPOPolicy.fused_wide_heads = True would take it on the fused kernels"
    if F.wide_ranks_would_take(pol, batch_size):
        return "; update_mode='fused' with PPOPolicy.fused_wide_ranks = True would take it on the fused kernels"
    return ""


class FusedPolicyUpdate(FusedEpoch):
    """Host driver of K12 (csrc/ppo_update.hip): one epoch of PPO._ppo_batch_train (ppo.py:2274-2485) for an MLP
    actor/critic."""

    @staticmethod
    def unsupported_reason(pol, batch_size, opt=None):
        """'' when the fused kernels cover this policy, else why not (the torch path is used then).  opt: the opt-ins the
        question is asked under (None: the policy's own, FusedOptIns.of)."""
        if pol.using_lstm or pol.agent_grouping:
            return "LSTM / grouped (MAT) policies are not covered by the fused MLP update"
        if opt is None:
            opt = FusedOptIns.of(pol)
        desc, why = describe_policy(pol, opt)
        if desc is None:
            return why
        a, c = desc.actor, desc.critic
        if batch_size < 2:
            return "batch size < 2"
        if desc.wide:
            pair = f"wide pair (actor {a.hidden}, critic {c.hidden})"
            if max(a.in_dim, c.in_dim) > 64 and not opt.wide_inputs:
                hint = "; PPOPolicy.fused_wide_inputs = True takes in_dim <= 128" if max(a.in_dim, c.in_dim) <= 128 else ""
                return f"{pair}: in_dim {a.in_dim} / {c.in_dim} > 64 (the split-wgrad chain's panels cover in_dim <= 64){hint}"
            if opt.wide_shapes:
                if max(a.in_dim, c.in_dim) > 512:
                    return (f"{pair}: in_dim {a.in_dim} / {c.in_dim} > 512 (with fused_wide_shapes the split-wgrad chain's panels "
                            "cover in_dim <= 512)")
                if batch_size > 1024:
                    return (f"{pair}: batch size {batch_size} > 1024 (with fused_wide_shapes the split-wgrad chain covers batch "
                            "sizes <= 1024)")
            else:
                if max(a.in_dim, c.in_dim) > 128:
                    return (f"{pair}: in_dim {a.in_dim} / {c.in_dim} > 128 (with fused_wide_inputs the split-wgrad chain's panels "
                            "cover in_dim <= 128)")
                if batch_size > 512:
                    return f"{pair}: batch size {batch_size} > 512 (the split-wgrad chain covers batch sizes <= 512)"
            if split_wgrad_mode() == "0":
                return f"{pair}: PPOAF_SPLIT_WGRAD=0, and the wide pair has no slab form"
            if mpi_utils.get_num_procs() > 1 and not opt.wide_ranks:
                return f"{pair}: single rank only for now ({mpi_utils.get_num_procs()} ranks)"
        # what the library itself refuses (depth, in_dim, the row-tile body's LDS): host-only, nothing is launched
        q = _lib.PpoUpdateArgs()
        q.actor, q.critic, q.bucket_total = a, c, a.size + c.size
        q.head_kind, q.B, q.batch_stride = desc.head, batch_size, batch_size
        q.row_pairs = opt.wide_bits if desc.wide else 0
        set_action_slices(q, desc.slices)
        if _lib.load().ppoaf_ppo_update_check(C.byref(q)) != 0:
            return _lib.load().ppoaf_last_error().decode("utf-8", "replace")
        return ""

    @staticmethod
    def fused_mode_would_take(pol, batch_size):
        """True for a policy that is refused only because `fused_wide_critic` is off (what "auto" says under verbose)."""
        return _would_take(FusedPolicyUpdate, pol, batch_size, "wide_critic")

    @staticmethod
    def wide_heads_would_take(pol, batch_size):
        """True for a policy that is refused only because `fused_wide_heads` is off -- under "auto", together with
        `fused_wide_critic` (what `verbose` adds to the refusal)."""
        return _would_take(FusedPolicyUpdate, pol, batch_size, "wide_heads", "wide_critic")

    @staticmethod
    def wide_ranks_would_take(pol, batch_size):
        """True for a policy that is refused only because `fused_wide_ranks` is off: a wide pair on N > 1 ranks -- under
        "auto", together with `fused_wide_critic` (what `verbose` adds to the refusal)."""
        return mpi_utils.get_num_procs() > 1 and _would_take(FusedPolicyUpdate, pol, batch_size, "wide_ranks", "wide_critic")

    def __init__(self, ppo, policy_id):
        super().__init__(ppo, policy_id)
        pol = self.pol
        dev = pol.device
        split_wgrad_mode()             # (a value that is none of the switch's is an error before anything is described or opened)
        opt = FusedOptIns.of(pol)
        self.head, self.action_slices, self.actor_desc, self.critic_desc, self.wide = describe_policy(pol, opt)[0]
        # the wide pair's option bits (read here, once: the args and the workspace are built from them)
        self.wide_bits = opt.wide_bits if self.wide else 0
        self.n_wg = (self.B + K.UPDATE_ROWS_PER_WG - 1) // K.UPDATE_ROWS_PER_WG
        total = pol.policy_params.numel()
        # (a wide pair has no slab form: a placeholder for the args' pointer instead of n_wg x 0.75 M floats nothing reads)
        self.slabs = torch.zeros((1, 4) if self.wide else (self.n_wg, total), dtype=torch.float32, device=dev)
        _init_normaliser(self)
        self.loss_partials = torch.zeros(2, self.n_wg, 8, dtype=torch.float32, device=dev)
        self.rows = None
        if self.wide and self.world > 1:
            # No K17 route for a wide pair: with a K17 launch between its wgrad and Adam launches, ranks that shared one GPU
            # ran K17's bounded wait out; the cause is not known.  The all-reduce route runs whatever
            # PPOAF_GRAD_EXCHANGE asks for.  (One rank rehearsing the N > 1 path waits for nobody and keeps its exchange.)
            self.xchg, self.xchg_reason = None, "a wide pair's gradients go through the all-reduce: no K17 route for it"
        else:
            self._open_exchange(total)
        # the fused tail launch of the split-wgrad chain (csrc/ppo_update_tail.hip) carries the exchange as a phase of
        # every weight-gradient job (one exchange group per workgroup, job-major tiles in the slots: an object of its own
        # again; at most 512 workgroups = the flag words of one exchange object): two launches per mini-batch on N > 1 ranks too.
        self.xchg_sp = None
        if self.xchg is not None and _switch("PPOAF_FUSED_TAIL", "1") != "0" \
                and split_wgrad_mode() != "0" and self._split_blocks() <= 512 \
                and max(self.actor_desc.in_dim, self.critic_desc.in_dim) <= 64 and self.B <= 512:
            self.xchg_sp, why = peer_exchange.open_exchange(self._tail_exchange_floats(), dev)
            if self.xchg_sp is not None and self.xchg_sp.status()[2] == 3:      # (the same kind on every rank: a collective choice)
                self.xchg_sp.close()
                self.xchg_sp, why = None, "coarse-grained slots need fences, which the fused tail launch does not use"
            if self.xchg_sp is None:
                self.xchg_reason += f"; fused-tail exchange refused ({why})"
        self.split, self.split_reason = self._split_wanted()

    def drop_peer_exchange(self, why):
        super().drop_peer_exchange(why)
        # the all-reduce loops run the slab chain -- but for a wide pair, which has none: its split-wgrad chain goes on with
        # the all-reduce between wgrad and Adam (_split_wanted)
        self.split, self.split_reason = self._split_wanted()
        self._split_space = None

    def _split_blocks(self):
        """Workgroups of ppoaf_ppo_update_wgrad for this policy's shapes (csrc/ppo_update_dev.hpp: split_wgrad_blocks)."""
        def jobs(d):
            t = d.hidden // 16
            return (d.depth - 1) * t * ((t + 1) // 2) + t * (((d.in_dim + 15) // 16 + 1) // 2) + 1
        return 8 * ((jobs(self.actor_desc) + jobs(self.critic_desc) + 7) // 8)

    def _tail_exchange_floats(self):
        """Floats of one slot of the fused tail's exchange (csrc/ppo_update_tail.hip: tail_exchange_floats): job-major
        16 x 32 tiles + 16 bias sums per workgroup, then the two networks' output segments (each padded to 4)."""
        def seg(d):
            sz_w0 = (d.hidden * d.in_dim + 3) // 4 * 4
            return d.size - (sz_w0 + d.hidden + (d.depth - 1) * (d.hidden * d.hidden + d.hidden))
        return self._split_blocks() * 528 + sum((seg(d) + 3) // 4 * 4 for d in (self.actor_desc, self.critic_desc))

    def _split_wanted(self):
        """
        (bool, why): the split-wgrad chain (fwd_bwd publishes activation / dz panels, ppoaf_ppo_update_wgrad forms the complete
        weight gradients) instead of weight-gradient slabs + the slab reduce.  PPOAF_SPLIT_WGRAD = auto | 1 | 0; auto =
        shapes the panels cover and, on N > 1 ranks, a K17 exchange plus a 256-wide network: the exchange is then a launch
        of its own between wgrad and Adam (four launches), which beats the slab chain's fused reduce + exchange launch only
        where the split saves more than a launch costs (<8,16>: 46.5 + 6.9 against 59 us; <8,8>: 17.8 + 5.1 against 21.4).
        """
        mode = split_wgrad_mode()
        if self.wide:
            return True, ""            # (the only form a wide pair has: unsupported_reason has refused everything else)
        if mode == "0":
            return False, "off (PPOAF_SPLIT_WGRAD=0)"
        if max(self.actor_desc.in_dim, self.critic_desc.in_dim) > 64 or self.B > 512:
            return False, "the panels cover in_dim <= 64 and batch sizes <= 512"
        if self.multi:
            if self.xchg is None:
                return False, "N > 1 without K17: the all-reduce loops run the slab chain"
            if self.xchg_sp is None and mode != "1" and max(self.actor_desc.hidden, self.critic_desc.hidden) < 256:   # (no fused-tail exchange)
                return False, "N > 1, no exchange for the wgrad launch and no 256-wide network: the slab reduce launch carries K17"
        return True, ""

    def description(self):
        """One line for `verbose`: the chain a mini-batch runs and, on the split-wgrad chain, the row stride of each
        network's layer-0 panel."""
        a, c = self.actor_desc, self.critic_desc
        line = f"K12 for (actor {a.hidden}, critic {c.hidden}), in_dim {a.in_dim} / {c.in_dim}"
        line += f", {a.out_dim} actor outputs (fused_wide_heads): " if a.out_dim > 8 else ": "
        if not self.split:
            return line + f"slab chain ({self.split_reason})"
        tail = self.tail_reason()
        line += "split-wgrad chain, " + ("fused tail" if tail == "" else f"wgrad and Adam launches ({tail})")
        if self.wide and self.multi and (self.world > 1 or FusedOptIns.of(self.pol).wide_ranks):
            # (one rank rehearsing the N > 1 path without the opt-in: the line it always had)
            line += "; " + self.exchange_route()
        return line + (f"; layer-0 panel stride {panel_stride(a.in_dim)} (actor) / {panel_stride(c.in_dim)} (critic) floats"
                       f"{', fused_wide_shapes' if self.wide_bits & _lib.SPLIT_WIDE_SHAPES else ', fused_wide_inputs' if self.wide_bits else ''}")

    def exchange_route(self):
        """N > 1, a wide pair: the route its mini-batch takes between the wgrad and the Adam launch (description())."""
        if self.xchg is not None:        # (only one rank rehearsing the N > 1 path holds an exchange: __init__)
            return "N > 1 rehearsed on one rank: fwd_bwd, wgrad, a K17 launch with no peer, Adam on its clip norms"
        # (which loop issues it is settled at the first epoch, by a vote of the ranks: rccl_comm -- not asked here)
        return (f"N > 1 ({self.world} ranks): all-reduce route -- fwd_bwd, wgrad, all-reduce, Adam with its norm pass: four "
                f"launches and a collective, eager ({self.xchg_reason})")

    def gradient_only(self, args, timing_events=(None, None)):
        """fwd_bwd + the launch that completes the gradient bucket (wgrad / slab reduce) of ONE mini-batch, no optimiser step:
        what tests and bench probes compare.  The bookkeeping of that launch (totals, step counters) runs as usual."""
        lib, st, ref = self._lib, K.stream(), C.byref(args)
        _lib.check(lib.ppoaf_ppo_update_fwd_bwd_timed(ref, timing_events[0], timing_events[1], st), "ppo_update_fwd_bwd")
        if args.split_workspace:
            _lib.check(lib.ppoaf_ppo_update_wgrad(ref, st), "ppo_update_wgrad")
        else:
            _lib.check(lib.ppoaf_ppo_update_reduce(ref, 1, st), "ppo_update_reduce")

    # ---- the RCCL fallback of every driver (rccl_comm)
    _rccl_comm_cache = "unset"         # process-wide: libppoaf_hip's own RCCL communicator (or None)
    rccl_loop = "c"                    # "python": the fallback's per-mini-batch loop from Python (tests compare the two)

    # ---- split-wgrad chain, 256-wide networks: a row tile on a PAIR of workgroups (csrc/ppo_update_rowpair.hpp)
    row_pairs = True                   # False: one workgroup per 16-row tile (bitwise the same results; tests compare the two)
    pair_launches = 0                  # fwd_bwd launches issued with row pairs in this process (graph replays not counted)

    def pairs_reason(self):
        """'' when fwd_bwd runs the 256-wide networks' row tiles on workgroup pairs, else why not (a narrower actor beside
        such a critic keeps one workgroup per tile)."""
        if not self.row_pairs:
            return "off (row_pairs = False)"
        if getattr(self, "_pairs_disabled", ""):
            return "disabled after a failed launch: " + self._pairs_disabled
        if not self.split:
            return "the slab chain runs (" + self.split_reason + ")"
        a, c = self.actor_desc, self.critic_desc
        ok = lambda d: d.hidden == 256 and 2 <= d.depth <= 4
        if not (ok(c) and (a.hidden < 256 or ok(a))):          # (csrc/ppo_update_dev.hpp: pairs_run)
            return "no 256-wide critic of depth 2 .. 4 beside a 32-, 64- or 128-wide actor or a 256-wide actor of depth 2 .. 4"
        return ""

    # ---- fused tail of the split-wgrad chain: fwd_bwd -> wgrad + clip norms + Adam in one launch (two launches per mini-batch)
    _tail_ctl_bytes = "ppo_update_tail_ctl_bytes"

    def tail_reason(self):
        """'' when a mini-batch of the split-wgrad chain ends in ppoaf_ppo_update_wgrad_adam, else why it takes the
        wgrad and Adam launches.  PPOAF_FUSED_TAIL = 1 (default) | 0."""
        if self.wide:                  # (at every depth: the fused tail is not instantiated for a 512-wide critic)
            return "wide pair: the mini-batch ends in the wgrad and Adam launches"
        if _switch("PPOAF_FUSED_TAIL", "1") == "0":
            return "off (PPOAF_FUSED_TAIL=0)"
        if getattr(self, "_tail_disabled", ""):
            return "disabled after a failed launch: " + self._tail_disabled
        if not self.split:
            return "the slab chain runs (" + self.split_reason + ")"
        if self._split_blocks() > 512:
            return f"{self._split_blocks()} weight-gradient workgroups (a polling wave of the fused launch holds 512 records)"
        if self.multi and os.environ.get("PPOAF_SHARE_DEVICE", "0") == "1" and self._split_blocks() * self.world > 512:
            # (tests: R ranks time-share ONE GPU.  Every rank's launch waits for the other ranks' records, so all R launches must
            #  be resident together: 2 x 369 workgroups of a 256-wide critic are not)
            return f"{self.world} ranks share one device: {self._split_blocks()} workgroups each cannot all be resident at once"
        if self.multi and self.xchg_sp is None:
            return "N > 1 without an exchange for the fused tail launch (" + self.xchg_reason + ")"
        return ""

    _waits = (
        BoundedWait(
            on=lambda u: u.pairs_reason() == "", used="_pairs_used",
            word=lambda u: u._split_space[u._pair_region:u._pair_region + 4].view(torch.int32),
            disabled="_pairs_disabled", reason="a workgroup's partner did not answer in time",
            failure="ppo_update_fwd_bwd (row pairs): a wait for the partner workgroup's half ran out of time "
                    "(another process on this GPU?)",
            # the pairs' records are tagged with the mini-batch index
            region=lambda u: u._split_space[u._pair_region:] if u._split_space is not None and u._pair_region >= 0 else None),
        _TAIL_WAIT)

    # ------------------------------------------------------------------ args
    def _make_args(self, B):
        pol, ppo = self.pol, self.ppo
        buf = pol.buffer
        a = _lib.PpoUpdateArgs()
        a.actor, a.critic = self.actor_desc, self.critic_desc
        a.params = pol.policy_params.data_ptr(); a.grads = pol.policy_grads.data_ptr()
        a.exp_avg = pol.policy_exp_avg.data_ptr(); a.exp_avg_sq = pol.policy_exp_avg_sq.data_ptr()
        a.slabs = self.slabs.data_ptr(); a.bucket_total = pol.policy_params.numel()
        a.step_counts = pol.policy_step_counts.data_ptr(); a.lr = pol.policy_lr.data_ptr()
        a.norm_scratch = pol.policy_norm_scratch.data_ptr()
        a.beta1, a.beta2, a.adam_eps = 0.9, 0.999, 1e-5
        a.grad_scale = 1.0 / self.world
        a.max_norm = float(pol.gradient_clip) if pol.gradient_clip is not None else 0.0
        a.head_kind = self.head
        set_action_slices(a, self.action_slices)
        a.obs = self.tables["obs"].data_ptr()
        a.perm = self.rows.data_ptr(); a.row_map = None      # rows = row_map[perm], resolved once per epoch
        a.min_std = float(getattr(pol.actor.distribution, "min_std", 0.01))
        _loss_args(self, a, B)
        a.xcd_half = getattr(self, "xcd_half", 0)        # 1 / 2: beside the ICM chain (ppo.py: _ppo_icm_epoch_overlapped)
        a.split_workspace, a.split_workspace_bytes = None, 0
        # (args.row_pairs is a bit set: the row pairs, and a wide pair's wider inputs and larger batches -- never both, a wide
        #  pair runs no pairs)
        a.row_pairs = wide_bit = self.wide_bits
        if self.split:
            a.row_pairs = wide_bit | int(self.pairs_reason() == "")
            if self._split_space is None:            # sized once for the full batch size; a tail mini-batch needs less
                need = C.c_int64(0)
                a.row_pairs = wide_bit | int(self.row_pairs)    # (room for the pairs' records whether or not they stay switched on)
                _lib.check(self._lib.ppoaf_ppo_update_split_workspace_bytes(C.byref(a), C.byref(need)), "split_workspace_bytes")
                self._split_space = torch.zeros(int(need.value), dtype=torch.uint8, device=pol.device)
                off = C.c_int64(-1)
                _lib.check(self._lib.ppoaf_ppo_update_row_pairs_error_offset(C.byref(a), C.byref(off)), "row_pairs_error_offset")
                self._pair_region = int(off.value)   # -1: these shapes run no pairs
                assert self._pair_region >= 0 or self.pairs_reason() != "", "the library runs no pairs for shapes pairs_reason() accepts"
                a.row_pairs = wide_bit | int(self.pairs_reason() == "")
                blocks = int(self._lib.ppoaf_ppo_update_split_blocks(C.byref(a)))
                if pol.policy_norm_scratch.numel() < 6 + 2 * blocks:      # one pair of norm partials per wgrad workgroup
                    pol.policy_norm_scratch = torch.zeros(6 + 2 * blocks, dtype=torch.float64, device=pol.device)
                    a.norm_scratch = pol.policy_norm_scratch.data_ptr()
                if self.xchg_sp is not None:         # the Python twin of the slot layout must be the library's
                    _lib.check(self._lib.ppoaf_ppo_update_tail_exchange_floats(C.byref(a), C.byref(need)), "ppo_update_tail_exchange_floats")
                    assert int(need.value) == self._tail_exchange_floats(), (int(need.value), self._tail_exchange_floats())
            a.split_workspace, a.split_workspace_bytes = self._split_space.data_ptr(), self._split_space.numel()
        return a

    def _signature(self):
        """Everything baked into captured launches; a change re-captures."""
        buf = self.pol.buffer
        return (buf.observations.data_ptr(), buf.num_transitions, self.rows.data_ptr(), self.tables["obs"].data_ptr(),
                getattr(self, "xcd_half", 0)) + _loss_signature(self)

    # ----------------------------------------------------------------- epoch
    def _epoch_inputs(self, N):
        pol, ppo = self.pol, self.ppo
        buf = pol.buffer
        # one dependent load less per mini-batch: the kernels read the buffer row directly
        if self.rows is None or self.rows.numel() != N:
            self.rows = torch.empty(N, dtype=torch.int64, device=pol.device)
            self._graphs.clear()
        torch.index_select(buf.row_map, 0, self.perm, out=self._rows32(N))
        self.rows.copy_(self._rows32(N))
        self._gather_tables(dict(obs=buf.observations, critic_obs=buf.critic_observations, raw_actions=buf.raw_actions,
                                 advantages=buf.advantages, log_probs=buf.log_probs, rewards_to_go=buf.rewards_to_go))
        nb = (N + self.B - 1) // self.B
        if ppo.normalize_values:
            local = K.minibatch_moments(buf.rewards_to_go.view(-1), self.perm, buf.row_map, self.B)
            if self.multi:
                allr = mpi_utils.allgather_records(local.reshape(-1)).view(self.world, nb, 3)
                rec = allr.permute(1, 0, 2).contiguous()
            else:
                rec = local.view(nb, 1, 3)
            if self.records is None or self.records.shape != rec.shape:
                self.records = torch.empty_like(rec)
                self._graphs.clear()
            self.records.copy_(rec)
            _seed_normaliser(self)
        if ppo.normalize_adv:
            if self.adv_records is None or self.adv_records.shape[0] != nb:
                self.adv_records = torch.empty(nb, 3, dtype=torch.float64, device=pol.device)
                self._graphs.clear()
            K.minibatch_moments(buf.advantages.view(-1), self.perm, buf.row_map, self.B, out=self.adv_records)

    def _rows32(self, N):
        t = getattr(self, "_rows_i32", None)
        if t is None or t.numel() != N:
            t = self._rows_i32 = torch.empty(N, dtype=torch.int32, device=self.pol.device)
        return t

    def _epoch_state(self):
        pol = self.pol
        return [pol.policy_params, pol.policy_exp_avg, pol.policy_exp_avg_sq, pol.policy_step_counts, pol.policy_norm_scratch,
                self.vn_mean, self.vn_var, self.vn_count, pol.buffer.values]

    _chunk = _chunk_with_offsets
    _publish = _publish_normaliser

    def _one(self, args):
        """One mini-batch: 3 launches (+ the gradient all-reduce on N > 1).  This is the eager path of
        multi-rank runs, so the per-call Python overhead is kept minimal: raw ctypes handles, the
        stream pointer looked up once per call."""
        lib = self._lib
        st = K.stream()
        ref = C.byref(args)
        single = not self.multi
        rc = lib.ppoaf_ppo_update_fwd_bwd(ref, st)
        if args.row_pairs & _lib.SPLIT_ROW_PAIRS:
            self._pairs_used = True
            FusedPolicyUpdate.pair_launches += 1
        if rc == 0 and args.split_workspace:
            # split-wgrad chain: complete weight gradients from the published panels, then clip + Adam
            if self.tail_reason() == "":
                # fused tail (csrc/ppo_update_tail.hip): weight gradients, [N > 1: the K17 exchange of every job's sums,]
                # clip norms and clip + Adam in ONE launch
                if single:
                    rc = lib.ppoaf_ppo_update_wgrad_adam(ref, self._tail_ctl_ptr(args), self.tail_wait_seconds, st)
                else:
                    rc = lib.ppoaf_ppo_update_wgrad_adam_exchange(ref, self._tail_ctl_ptr(args), self.tail_wait_seconds,
                                                                 self.xchg_sp.handle, self.xchg_sp.wait_seconds, st)
                self._tail_used = True
                if rc != 0:
                    _lib.check(rc, "ppo_update_wgrad_adam")
                return
            rc = lib.ppoaf_ppo_update_wgrad(ref, st)
        elif rc == 0 and self.xchg is not None and self.pol.policy_grads.numel() <= 256 * 1024:
            # slab reduce + K17 exchange in one launch (sums travel from registers to the exchange slot)
            rc = lib.ppoaf_ppo_update_reduce_exchange(ref, self.xchg.handle, self.xchg.wait_seconds, st) \
                or lib.ppoaf_ppo_update_adam_exchanged(ref, self.xchg.handle, st)
            if rc != 0:
                _lib.check(rc, "ppo_update")
            return
        elif rc == 0:
            rc = lib.ppoaf_ppo_update_reduce(ref, 1 if single else 0, st)
        if rc == 0 and self.xchg is not None:
            # K17: summed gradients + both clip norms in one launch, then Adam without a norm pass
            g = self.pol.policy_grads
            self.xchg.allreduce(g, g, split_floats=self.actor_desc.size, norm_scale=args.grad_scale,
                                norm_out=self.pol.policy_norm_scratch, stream=st)
            rc = lib.ppoaf_ppo_update_adam(ref, 2, st)
        elif rc == 0 and args.split_workspace and single:
            rc = lib.ppoaf_ppo_update_adam(ref, 3, st)       # (the wgrad launch left both clip norms)
        else:
            if rc == 0 and not single:
                mpi_utils.allreduce_sum_(self.pol.policy_grads)
            if rc == 0:
                rc = lib.ppoaf_ppo_update_adam(ref, 0 if single else 1, st)
        if rc != 0:
            _lib.check(rc, "ppo_update")

    def _chain_allreduce(self, ref, comm, k, st):
        # 5 launches per mini-batch without returning to Python (host cost below the GPU's)
        _lib.check(self._lib.ppoaf_ppo_update_chain_allreduce(ref, comm, k, st), "ppo_update_chain_allreduce")


# ======================================================================================
# K14: fused ICM update
# ======================================================================================
def _describe_icm(icm, action_dtype):
    """
    Topology fields of an ICM living in one flat bucket, or (None, reason): IcmUpdateArgs' for the one-width topology
    (csrc/icm_update.hip), else IcmShapesArgs' plus `general=True` for an ICM whose encoder, encoding and models have
    widths of their own (csrc/icm_update_shapes.hip).
    """
    topo, _ = _describe_icm_one_width(icm, action_dtype)
    if topo is not None:
        return topo, ""
    return _describe_icm_shapes(icm, action_dtype)


def _icm_bucket_marks(icm, groups):
    """Bucket offsets of the layer groups when the bucket is the groups' parameters in order, each padded to 4 floats:
    (marks, total), or (None, reason)."""
    base = icm.flat_params.data_ptr()
    off, marks = 0, []
    for group in groups:
        marks.append(off)
        for m in group:
            for p in (m.weight, m.bias):
                if (p.data_ptr() - base) // 4 != off:
                    return None, "parameter layout differs from the kernel's layer table"
                off += (p.numel() + 3) // 4 * 4
    if off != icm.flat_params.numel():
        return None, "the ICM holds parameters the fused kernel does not know about"
    return marks, off


def _icm_action_slices(icm):
    """MultiDiscrete ICM actions on the shapes chain (csrc/icm_update_shapes.hip, n_action_slices): (slices, total classes,
    "") or (0, 0, reason).  The kernels take k <= 8 equal slices of n >= 2 classes, k n <= 16."""
    nvec = [int(n) for n in (getattr(icm, "action_nvec", None) or [])]
    if not nvec:
        return 0, 0, "multi-discrete actions without class counts (nvec)"
    if len(set(nvec)) != 1:
        return 0, 0, (f"multi-discrete class counts {nvec} differ: the reference's forward-model one-hot (icm.py:198-211) is "
                      "only well-formed for equal class counts")
    if nvec[0] < 2:
        return 0, 0, f"multi-discrete class count of {nvec[0]}: every slice needs at least 2 classes"
    if len(nvec) > 8:
        return 0, 0, f"multi-discrete actions of {len(nvec)} slices: the fused ICM kernels take at most 8"
    if sum(nvec) > 16:
        return 0, 0, f"multi-discrete actions of {sum(nvec)} classes in all: the fused ICM kernels take at most 16"
    return len(nvec), sum(nvec), ""


def _icm_action_widths_reason(A, Ain, wide_actions):
    """'' when Discrete / Box action widths are the kernels': [1, 8], or [1, WIDE_HEAD_MAX] with wide_actions."""
    top = WIDE_HEAD_MAX if wide_actions else 8
    return "" if 1 <= A <= top and 1 <= Ain <= top else f"action widths ({A}, {Ain}) must be in [1, {top}]"


def _describe_icm_general(icm, action_dtype, enc, multi_discrete, wide_actions):
    """The body of _describe_icm_shapes (enc: the encoder's four Linear layers) and of _describe_icm_identity (enc: ()).
    Without an encoder the models work on the observation itself: D = O, and the texts say O."""
    slices = 0
    if action_dtype == "multi-discrete":
        if not multi_discrete:
            return None, "multi-discrete actions are not covered by the fused ICM update"
        slices, classes, why = _icm_action_slices(icm)
        if why:
            return None, why
    elif action_dtype not in ("discrete", "continuous"):
        return None, "unsupported action space for the fused ICM update"
    inv = [m for m in icm.inv_model.sequential_net.modules() if isinstance(m, nn.Linear)]
    fwd = [m for m in icm.forward_model.sequential_net.modules() if isinstance(m, nn.Linear)]
    widths = (32, 64, 128)
    E = 0
    if enc:
        E, O, D = enc[0].out_features, enc[0].in_features, enc[3].out_features
        if E not in widths:
            return None, f"encoder width {E} is not an instantiated width {widths}"
        if [(m.in_features, m.out_features) for m in enc] != [(O, E), (E, E), (E, E), (E, D)]:
            return None, "encoder layers must be O -> E -> E -> E -> D"
        if not 1 <= D <= 128:
            return None, f"encoded dim {D} must be in [1, 128]"
        if not 1 <= O <= 1024:
            return None, f"observation size {O} must be in [1, 1024]"
    if len(inv) < 2 or len(fwd) < 2 or len(inv) > 4 or len(fwd) > 4:
        return None, "inverse / forward model need 1..3 hidden layers"
    if not enc:
        O = D = fwd[-1].out_features
        if not 1 <= O <= 128:
            return None, f"identity encoder: observation size O = {O} is above the fused kernels' limit of 128"
    Mi, Mf = inv[0].out_features, fwd[0].out_features
    if Mi not in widths or Mf not in widths:
        return None, f"inverse / forward model widths ({Mi}, {Mf}) are not instantiated widths {widths}"
    A, Ain = inv[-1].out_features, fwd[0].in_features - D
    want_inv = [(2 * D, Mi)] + [(Mi, Mi)] * (len(inv) - 2) + [(Mi, A)]
    want_fwd = [(D + Ain, Mf)] + [(Mf, Mf)] * (len(fwd) - 2) + [(Mf, D)]
    if [(m.in_features, m.out_features) for m in inv] != want_inv or \
            [(m.in_features, m.out_features) for m in fwd] != want_fwd:
        return None, ("inverse / forward model layers do not follow 2D -> Mi .. -> A / D + Ain -> Mf .. -> D" if enc else
                      "inverse / forward model layers do not follow 2 O -> Mi .. -> A / O + Ain -> Mf .. -> O")
    if slices:
        if (A, Ain) != (classes, classes):
            return None, f"action widths ({A}, {Ain}) are not the {classes} classes of the multi-discrete action space"
    elif _icm_action_widths_reason(A, Ain, wide_actions):
        return None, _icm_action_widths_reason(A, Ain, wide_actions)
    if action_dtype == "discrete" and Ain != A:
        return None, "unsupported action space for the fused ICM update"
    acts = {_activation_code(a) for a in (icm.activation, *([icm.obs_encoder.activation] if enc else []),
                                           icm.inv_model.activation, icm.forward_model.activation)}
    if len(acts) != 1 or None in acts:
        return None, "activation is not one shared ReLU / LeakyReLU(0.01) / Tanh"
    if split_wgrad_mode() == "0":
        return None, "PPOAF_SPLIT_WGRAD=0: the chain for these ICM shapes has no slab form"
    marks, total = _icm_bucket_marks(icm, (enc, inv, fwd))       # (an encoder of size 0: enc_offset == inv_offset)
    if marks is None:
        return None, total
    topo = dict(general=True, obs_dim=O, enc_hidden=E, enc_dim=D, inv_hidden=Mi, fwd_hidden=Mf, action_dim=A, fwd_action_dim=Ain,
                depth_inv=len(inv) - 1, depth_fwd=len(fwd) - 1, activation=acts.pop(), discrete=int(action_dtype == "discrete"),
                enc_offset=marks[0], inv_offset=marks[1], fwd_offset=marks[2], bucket_total=total)
    if not enc:
        topo.update(identity=True)
    if slices:
        topo.update(discrete=1, n_action_slices=slices)
    elif max(A, Ain) > 8:
        topo.update(n_action_slices=_lib.ICM_WIDE_ACTIONS)
    return topo, ""


def _describe_icm_shapes(icm, action_dtype, multi_discrete=False, wide_actions=False):
    """IcmShapesArgs topology fields (+ general=True) of an ICM, or (None, reason).  Covered: encoder O -> E -> E -> E -> D,
    inverse 2D -> Mi (x 1..3) -> A, forward D + Ain -> Mf (x 1..3) -> D; E, Mi, Mf in (32, 64, 128), 1 <= D <= 128.
    multi_discrete: MultiDiscrete actions are described as well (n_action_slices; _icm_action_slices has the limits).
    wide_actions (the opt-in PPOPolicy.fused_wide_icm_actions): Discrete / Box widths of 9 .. WIDE_HEAD_MAX are described too;
    the topology carries _lib.ICM_WIDE_ACTIONS only when a width is above 8."""
    from .networks.icm import ICM, LinearObservationEncoder
    if not isinstance(icm, ICM):
        return None, "not an ICM"
    if not isinstance(icm.obs_encoder, LinearObservationEncoder):
        return None, ("the identity encoder (encoded_obs_dim = 0) is not covered: the fused kernels need a "
                      "LinearObservationEncoder")
    e = icm.obs_encoder
    return _describe_icm_general(icm, action_dtype, [e.enc_1, e.enc_2, e.enc_3, e.enc_4], multi_discrete, wide_actions)


def _describe_icm_identity(icm, action_dtype, multi_discrete=False, wide_actions=False):
    """IcmShapesArgs topology fields (+ general=True, identity=True) of an ICM whose encoder is nn.Identity()
    (encoded_obs_dim = 0), or (None, reason).  The kernels read it as enc_hidden = 0, enc_dim = obs_dim = O and an encoder
    of size 0 (enc_offset == inv_offset).  Covered: 1 <= O <= 128, inverse 2 O -> Mi (x 1..3) -> A, forward O + Ain -> Mf
    (x 1..3) -> O; Mi, Mf in (32, 64, 128).  multi_discrete / wide_actions: as _describe_icm_shapes."""
    from .networks.icm import ICM
    if not isinstance(icm, ICM):
        return None, "not an ICM"
    if not isinstance(icm.obs_encoder, nn.Identity):
        return None, "not an identity encoder (encoded_obs_dim > 0)"
    return _describe_icm_general(icm, action_dtype, (), multi_discrete, wide_actions)


def describe_icm_chain(icm, action_dtype, multi_discrete=False, wide_actions=False):
    """Which K14 chain trains `icm`: the one-width description, else the one for widths of their own, else the identity
    encoder's; (topology, "") or (None, reason of the describer that matches the ICM's encoder type).
    multi_discrete (the opt-in PPOPolicy.fused_shared_icm): an ICM over MultiDiscrete actions of equal class counts is
    described too -- always on the shapes chain or the identity form, whose kernels have the multi-categorical head; the
    one-width chain is not asked.  Without it such an ICM is refused as before.
    wide_actions (the opt-in PPOPolicy.fused_wide_icm_actions): an ICM that the describers refuse is asked again with
    Discrete / Box widths up to WIDE_HEAD_MAX on the shapes chain or the identity form -- a one-width ICM (128/128/128) with
    such actions too: the one-width kernels keep 8.  Whatever is described without it is described exactly so with it."""
    if multi_discrete and action_dtype == "multi-discrete":
        if isinstance(getattr(icm, "obs_encoder", None), nn.Identity):
            return _describe_icm_identity(icm, action_dtype, True)
        return _describe_icm_shapes(icm, action_dtype, True)
    topo, why = _describe_icm(icm, action_dtype)
    if topo is not None:
        return topo, ""
    if isinstance(getattr(icm, "obs_encoder", None), nn.Identity):
        return _describe_icm_identity(icm, action_dtype, wide_actions=wide_actions)
    if wide_actions and action_dtype in ("discrete", "continuous"):
        return _describe_icm_shapes(icm, action_dtype, wide_actions=True)
    return None, why


def describe_policy_icm(pol, opt=None):
    """Which K14 chain trains the policy's ICM under the opt-ins `opt` (None: the policy's own): describe_icm_chain's
    (topology, "") or (None, reason).  An agent-shared ICM (FusedIcmUpdate._shared) is described with its own action dtype
    -- the policy's is the agents' "discrete", the ICM's is what it trains on -- and its multi-categorical head."""
    if opt is None:
        opt = FusedOptIns.of(pol)
    if FusedIcmUpdate._shared(pol, opt):
        return describe_icm_chain(pol.icm_model, pol.icm_model.action_dtype, multi_discrete=True)
    return describe_icm_chain(pol.icm_model, pol.action_dtype, wide_actions=opt.wide_icm_actions)


def icm_scratch_floats(topo, rows):
    """(act_scratch, denc_scratch) floats of either K14 chain for `rows` rows (include/ppoaf_hip.h)."""
    bpad = (rows + 15) // 16 * 16
    if topo.get("identity"):                     # the two observation panels; no d(enc) (a token allocation)
        return 2 * bpad * ((topo["obs_dim"] + 15) // 16 * 16), 4
    if topo.get("general"):
        dp = (topo["enc_dim"] + 15) // 16 * 16
        return 2 * bpad * (3 * topo["enc_hidden"] + dp), 4 * bpad * dp
    return 8 * bpad * topo["hidden"], 4 * bpad * topo["hidden"]


def icm_topology_args(topo):
    """The args struct of the chain `topo` selects, topology fields set."""
    a = _lib.IcmShapesArgs() if topo.get("general") else _lib.IcmUpdateArgs()
    for k, v in topo.items():
        if k not in ("general", "identity"):
            setattr(a, k, v)
    return a


def _describe_icm_one_width(icm, action_dtype):
    """IcmUpdateArgs topology fields of an ICM living in one flat bucket, or (None, reason)."""
    from .networks.icm import ICM, LinearObservationEncoder
    if not isinstance(icm, ICM) or not isinstance(icm.obs_encoder, LinearObservationEncoder):
        return None, "ICM with a LinearObservationEncoder is what the fused kernels cover"
    enc = [icm.obs_encoder.enc_1, icm.obs_encoder.enc_2, icm.obs_encoder.enc_3, icm.obs_encoder.enc_4]
    inv = [m for m in icm.inv_model.sequential_net.modules() if isinstance(m, nn.Linear)]
    fwd = [m for m in icm.forward_model.sequential_net.modules() if isinstance(m, nn.Linear)]
    H, O = enc[0].out_features, enc[0].in_features
    if H not in (64, 128):
        return None, f"ICM width {H} is not an instantiated width (64, 128)"
    if any((m.in_features, m.out_features) != (H, H) for m in enc[1:]):
        return None, "encoder layers must share one width (encoded_obs_dim == encoder_hidden_size)"
    if len(inv) < 2 or len(fwd) < 2 or len(inv) > 4 or len(fwd) > 4:
        return None, "inverse / forward model need 1..3 hidden layers"
    A, Ain = inv[-1].out_features, fwd[0].in_features - H
    want_inv = [(2 * H, H)] + [(H, H)] * (len(inv) - 2) + [(H, A)]
    want_fwd = [(H + Ain, H)] + [(H, H)] * (len(fwd) - 2) + [(H, H)]
    if [(m.in_features, m.out_features) for m in inv] != want_inv or \
            [(m.in_features, m.out_features) for m in fwd] != want_fwd:
        return None, "inverse / forward model widths must equal the encoder width"
    if not (1 <= A <= 8 and 1 <= Ain <= 8):
        return None, f"action widths ({A}, {Ain}) must be in [1, 8]"
    if action_dtype not in ("discrete", "continuous") or (action_dtype == "discrete" and Ain != A):
        return None, "unsupported action space for the fused ICM update"
    acts = {_activation_code(a) for a in (icm.activation, icm.obs_encoder.activation, icm.inv_model.activation,
                                           icm.forward_model.activation)}
    if len(acts) != 1 or None in acts:
        return None, "activation is not one shared ReLU / LeakyReLU(0.01) / Tanh"
    marks, off = _icm_bucket_marks(icm, (enc, inv, fwd))
    if marks is None:
        return None, off
    return dict(obs_dim=O, hidden=H, action_dim=A, fwd_action_dim=Ain, depth_inv=len(inv) - 1,
                depth_fwd=len(fwd) - 1, activation=acts.pop(), discrete=int(action_dtype == "discrete"),
                enc_offset=marks[0], inv_offset=marks[1], fwd_offset=marks[2], bucket_total=off), ""


class FusedIcmUpdate(FusedEpoch):
    """
    Host driver of K14 (csrc/icm_update.hip): one epoch of PPO._icm_batch_train (ppo.py:2487-2567).
    Per mini-batch: fwd_bwd (3 launches) -> reduce [+ Adam]; with more ranks reduce -> all-reduce ->
    K11 Adam.  On a single rank `graph_chunk` mini-batches are captured into a hipGraph and replayed
    (all launches read the device cursor).  An ICM with widths of its own (`topo["general"]`) runs the same protocol on
    csrc/icm_update_shapes.hip: ppoaf_icm_shapes_fwd_bwd -> ppoaf_icm_shapes_wgrad, split-wgrad form only; so does an ICM
    with an identity encoder (`topo["identity"]`), whose fwd_bwd is the models launch alone.

    Agent-grouped (MAT) policies without agent_shared_icm (ppo.py:2540-2545, "case 3"): the ICM samples of a mini-batch of
    n grouped rows are its n A (row, agent) pairs in row-major order.  The epoch's tables are [N, A, .] in shuffled order,
    which read as [N A, .] are those samples in mini-batch order, so the kernels run with inputs_in_batch_order = 1,
    B = n A and batch_stride = batch_size A: icm_rows (csrc/icm_update_dev.hpp) then takes row cursor * batch_stride + s of
    the tables and reads neither `perm` nor `row_map` (they index the buffer's grouped rows, not the samples: NULL here),
    and n_rows = N A only bounds the tables.  `self.B`, the tail and the cursor keep counting grouped rows / mini-batches.

    Agent-grouped policies with agent_shared_icm (ppo.py:2520-2538, "case 2"), behind the opt-in `pol.fused_shared_icm`: one
    ICM sample per grouped row, its observation the group's observations side by side in the order of the policy's current
    agent_idxs, its action the group's classes in that order -- MultiDiscrete([n] * A), topo["n_action_slices"] = A.  The
    epoch's gathered tables [N, A, .] are re-ordered along the agent axis by agent_idxs (taken at begin_epoch: the policy
    reshuffles it at every rollout) and read as [N, A O], [N, A O] and int64 [N, A]; self.A = 1, so B and batch_stride
    count grouped rows, inputs_in_batch_order = 1, perm / row_map NULL and n_rows = N.
    """

    n_totals = 2
    min_tail_rows = 1

    @staticmethod
    def unsupported_reason(pol, batch_size=None, opt=None):
        """'' or why the torch path trains the policy's ICM.  opt: the opt-ins the question is asked under (None: the
        policy's own)."""
        if opt is None:
            opt = FusedOptIns.of(pol)
        if not pol.enable_icm:
            return "no ICM"
        shared = FusedIcmUpdate._shared(pol, opt)
        if pol.agent_grouping and pol.agent_shared_icm and not shared:
            return ("agent_shared_icm: one ICM over the MultiDiscrete action space of the whole group (ppo.py:2520-2538) "
                    "is not covered, torch path")
        _, why = describe_policy_icm(pol, opt)
        if not why and pol.agent_grouping and not shared and batch_size is not None:
            A = FusedIcmUpdate._agents(pol, opt)
            if batch_size * A > 65536:
                return f"agent-grouped policy: batch_size x agents = {batch_size} x {A} ICM rows per mini-batch exceed 65536"
        return why

    @staticmethod
    def wide_actions_would_take(pol, batch_size=None):
        """True for an ICM that is refused only because `fused_wide_icm_actions` is off (what `verbose` adds to the refusal)."""
        refused = FusedIcmUpdate.unsupported_reason(pol, batch_size) != ""
        return refused and _would_take(FusedIcmUpdate, pol, batch_size, "wide_icm_actions")

    @staticmethod
    def _shared(pol, opt=None):
        """The agent-shared ICM of an agent-grouped policy on the fused kernels (opt-in: PPOPolicy.fused_shared_icm)."""
        return bool(getattr(pol, "agent_grouping", False) and pol.agent_shared_icm and (opt or FusedOptIns.of(pol)).shared_icm)

    @staticmethod
    def _agents(pol, opt=None):
        """ICM samples per buffer row: the group's agents for an agent-grouped policy (1 when they share one ICM), else 1."""
        if FusedIcmUpdate._shared(pol, opt):
            return 1
        return int(getattr(pol, "num_agents", 0) or len(pol.agent_ids)) if getattr(pol, "agent_grouping", False) else 1

    def __init__(self, ppo, policy_id):
        super().__init__(ppo, policy_id)
        pol = self.pol
        dev = pol.device
        opt = FusedOptIns.of(pol)                          # read once, as the refusal was: the opt-ins are set before the first epoch
        self.shared = self._shared(pol, opt)
        self.topo, _ = describe_policy_icm(pol, opt)
        self.general = bool(self.topo.get("general"))      # csrc/icm_update_shapes.hip: split-wgrad form only, no in-kernel waits
        self.A = self._agents(pol, opt)                    # ICM samples per buffer row (agent-grouped policies: the agents)
        rows = self.B * self.A                             # everything below is sized for a full mini-batch's samples
        nT = (rows + K.UPDATE_ROWS_PER_WG - 1) // K.UPDATE_ROWS_PER_WG
        total = self.topo["bucket_total"]
        self.slabs = None if self.general else torch.zeros(2 * nT, total, dtype=torch.float32, device=dev)
        n_act, n_denc = icm_scratch_floats(self.topo, rows)
        self.act_scratch = torch.zeros(n_act, dtype=torch.float32, device=dev)
        self.denc_scratch = torch.zeros(n_denc, dtype=torch.float32, device=dev)
        self.loss_partials = torch.zeros(nT + 1, 2, dtype=torch.float32, device=dev)    # + the step's Adam constants
        self._open_exchange(pol.icm_model.flat_grads.numel())
        # split-wgrad chain (csrc/icm_update.hip: icm_wgrad_kernel): PPOAF_SPLIT_WGRAD = auto (= 1) | 1 | 0.  The reduce entry
        # point keeps its contract, so graphs, K17 and the RCCL loop are the same with either form.
        self.split = split_wgrad_mode() != "0"

    def drop_peer_exchange(self, why):
        super().drop_peer_exchange(why)
        if not getattr(self, "_fuse_disabled", ""):
            self._fuse_disabled = why          # every rank runs the same three launches from here on

    def _make_args(self, B):
        pol, buf, opt = self.pol, self.pol.buffer, self.pol.icm_optim
        a = icm_topology_args(self.topo)
        icm = pol.icm_model
        a.params, a.grads = icm.flat_params.data_ptr(), icm.flat_grads.data_ptr()
        a.exp_avg, a.exp_avg_sq = opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr()
        if not self.general:
            a.slabs = self.slabs.data_ptr()
        a.step_count, a.lr = opt.step_count.data_ptr(), opt.lr.data_ptr()
        a.beta1, a.beta2, a.adam_eps = opt.betas[0], opt.betas[1], opt.eps
        a.grad_scale = 1.0 / self.world
        t = self.tables                        # per-epoch inputs in shuffled order (begin_epoch)
        a.obs, a.next_obs, a.actions = t["obs"].data_ptr(), t["next_obs"].data_ptr(), t["actions"].data_ptr()
        a.inputs_in_batch_order = 1
        if self.A > 1 or self.shared:
            # (row, agent) samples: the tables read as [N A, .]; perm / row_map are not the samples' (class comment).
            # Shared ICM: A = 1, the tables' rows are the N joined grouped rows
            a.perm, a.row_map, a.n_rows = None, None, self.perm.numel() * self.A
        else:
            a.perm, a.row_map, a.n_rows = self.perm.data_ptr(), buf.row_map.data_ptr(), buf.num_transitions
        a.cursor, a.B, a.batch_stride = self.cursor.data_ptr(), B * self.A, self.B * self.A
        a.icm_beta = float(pol.icm_beta)
        a.fused_adam = int(not self.multi)
        a.act_scratch, a.denc_scratch = self.act_scratch.data_ptr(), self.denc_scratch.data_ptr()
        a.loss_partials, a.totals = self.loss_partials.data_ptr(), self.totals.data_ptr()
        a.xcd_half = getattr(self, "xcd_half", 0)
        if self.general:
            if self._split_space is None:                # sized once, for the full batch size (a tail mini-batch needs less)
                need = C.c_int64(0)
                _lib.check(self._lib.ppoaf_icm_shapes_workspace_bytes(C.byref(a), C.byref(need)), "icm_shapes_workspace_bytes")
                self._split_space = torch.zeros(int(need.value), dtype=torch.uint8, device=pol.device)
            a.workspace, a.workspace_bytes = self._split_space.data_ptr(), self._split_space.numel()
            return a
        a.split_workspace, a.split_workspace_bytes = None, 0
        a.fuse_kernels = 0
        if self.split:
            # one launch for the encoder / model / encoder-backward kernels (csrc/icm_update.hip: icm_fused_kernel); its exchange
            # records sit at the start of the workspace, so the flag must not change once the workspace exists
            a.fuse_kernels = int(self.fuse_kernels and not getattr(self, "_fuse_disabled", ""))
            if self._split_space is None:                # sized once, for the full batch size (a tail mini-batch needs less)
                need = C.c_int64(0)
                _lib.check(self._lib.ppoaf_icm_update_split_workspace_bytes(C.byref(a), C.byref(need)), "icm_update_split_workspace_bytes")
                self._split_space = torch.zeros(int(need.value), dtype=torch.uint8, device=pol.device)
            self._split_fused_layout = a.fuse_kernels    # (switched off after a failed launch: the panels move to the front)
            a.split_workspace, a.split_workspace_bytes = self._split_space.data_ptr(), self._split_space.numel()
            self._fuses = a.fuse_kernels == 1 and self._lib.ppoaf_icm_update_fuses_kernels(C.byref(a)) == 1
        return a

    def _signature(self):
        pol, buf = self.pol, self.pol.buffer
        return (self.tables["obs"].data_ptr(), buf.observations.data_ptr(), buf.next_observations.data_ptr(),
                buf.actions.data_ptr(), buf.num_transitions, self.perm.data_ptr(), float(pol.icm_beta), getattr(self, "xcd_half", 0))

    fuse_kernels = True                # False: the three kernels as three launches (bitwise the same; tests compare the two)
    fused_launches = 0                 # single launches issued in this process (graph replays not counted)
    _REC_BYTES = 256 + 2 * 32 * 2 * 16384     # csrc/icm_update.hip: kIcmRecBytes

    def fuse_reason(self):
        """'' when a mini-batch's encoder / model / encoder-backward kernels run as one launch, else why not."""
        if self.general:
            return "the chain for ICMs with widths of their own has no single-launch form (and no bounded waits)"
        if not self.fuse_kernels:
            return "off (fuse_kernels = False)"
        if getattr(self, "_fuse_disabled", ""):
            return "disabled after a failed launch: " + self._fuse_disabled
        if not self.split:
            return "the slab chain runs (PPOAF_SPLIT_WGRAD=0)"
        self._args_for(self.B)
        return "" if getattr(self, "_fuses", False) else "hidden width other than 128, or no LDS room for the three phases"

    _FUSED_FAILURE = "icm_fused_kernel: a wait for the partner workgroup's records ran out of time (another process on this GPU?)"
    _waits = (BoundedWait(
        on=lambda u: u.fuse_reason() == "", used="_fused_used", word=lambda u: u._split_space[:4].view(torch.int32),
        disabled="_fuse_disabled", reason=_FUSED_FAILURE, failure=_FUSED_FAILURE,
        # the exchange records are tagged with the cursor (in the workspace's fused layout only)
        region=lambda u: u._split_space[:u._REC_BYTES] if u._split_space is not None and getattr(u, "_split_fused_layout", 0)
        else None),)

    def _epoch_inputs(self, N):
        buf = self.pol.buffer
        if not self.shared:
            self._gather_tables(dict(obs=buf.observations, next_obs=buf.next_observations, actions=buf.actions))
            return
        # case 2 (ppo.py:2520-2538; the torch path: PPO._icm_batch_train): gather [N, A, .] in shuffled order, then the agents
        # in the order of the policy's current agent_idxs, side by side in one row -- once per epoch, into tables that keep
        # their addresses (the captured launches read them)
        grouped = self._gather_tables(dict(obs=buf.observations, next_obs=buf.next_observations, actions=buf.actions),
                                      into="_grouped_tables")
        joined = self._epoch_tables("tables", N, {k: ((v[0].numel(),), v.dtype, v.device) for k, v in grouped.items()})
        order = self.ppo._scratch(f"icm_agent_order_{self.policy_id}", len(self.pol.agent_idxs), torch.int64)
        order.copy_(torch.as_tensor(np.asarray(self.pol.agent_idxs), dtype=torch.int64))
        for k, v in grouped.items():
            torch.index_select(v.reshape(N, buf.A, -1), 1, order, out=joined[k].view(N, buf.A, -1))

    def _one(self, args):
        lib, st, ref = self._lib, K.stream(), C.byref(args)
        if self.general:
            rc = lib.ppoaf_icm_shapes_fwd_bwd(ref, st)
            if rc == 0:
                rc = lib.ppoaf_icm_shapes_wgrad(ref, st)
        else:
            rc = lib.ppoaf_icm_update_fwd_bwd(ref, st)
            if args.fuse_kernels and getattr(self, "_fuses", False):
                self._fused_used = True
                FusedIcmUpdate.fused_launches += 1
            if rc == 0:
                rc = lib.ppoaf_icm_update_reduce(ref, st)
        if rc != 0:
            _lib.check(rc, "icm_update")
        if self.multi:
            g = self.pol.icm_model.flat_grads
            if self.xchg is not None:
                self.xchg.allreduce(g, g, stream=st)                                  # K17, in-graph
            else:
                mpi_utils.allreduce_sum_(g)
            self.pol.icm_optim.step(grad_scale=1.0 / self.world, max_norm=None)

    def _c_loop(self, args, n):
        # (the C-level RCCL loop is the one-width chain's: these shapes take _one's all-reduce branch)
        return False if self.general else super()._c_loop(args, n)

    def _chain_allreduce(self, ref, comm, k, st):
        opt = self.pol.icm_optim
        _lib.check(self._lib.ppoaf_icm_update_chain_allreduce(ref, comm, k, opt.norm_scratch.data_ptr(), opt.grad_norm.data_ptr(), st),
                   "icm_update_chain_allreduce")

    def _epoch_state(self):
        opt, icm = self.pol.icm_optim, self.pol.icm_model
        return [icm.flat_params, opt.exp_avg, opt.exp_avg_sq, opt.step_count]


# ======================================================================================
# K15: fused multi-agent-transformer update
# ======================================================================================
_MAT_PARAM_NAMES = (
    ["actor.action_encoder.0.weight", "actor.ln.weight", "actor.ln.bias"]
    + [f"actor.blocks.0.ln{i}.{p}" for i in (1, 2, 3) for p in ("weight", "bias")]
    + [f"actor.blocks.0.attn{i}.{n}.{p}" for i in (1, 2) for n in ("key_net", "query_net", "value_net", "proj")
       for p in ("weight", "bias")]
    + [f"actor.blocks.0.mlp.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")]
    + [f"actor.head.{i}.{p}" for i in (0, 2, 3) for p in ("weight", "bias")]
    + [f"critic.obs_encoder.{i}.{p}" for i in (0, 1) for p in ("weight", "bias")]
    + ["critic.ln.weight", "critic.ln.bias"]
    + [f"critic.blocks.0.ln{i}.{p}" for i in (1, 2) for p in ("weight", "bias")]
    + [f"critic.blocks.0.attn.{n}.{p}" for n in ("key_net", "query_net", "value_net", "proj") for p in ("weight", "bias")]
    + [f"critic.blocks.0.mlp.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")]
    + [f"critic.head.{i}.{p}" for i in (0, 2, 3) for p in ("weight", "bias")])


# per-agent observation widths of the MAT kernels (csrc/mat_update.hip): K15 and K16 stream rows wider than 32 through LDS in
# column chunks, up to 128; K20's entry point stops at 64
MAT_MAX_OBS = 128
MAT_INFER_MAX_OBS = 64


def _describe_mat(pol):
    """Topology + offset table of a MATPolicy's actor_critic for K15, or (None, reason)."""
    from .networks.multi_agent_transformer import MATActorCritic
    ac = getattr(pol, "actor_critic", None)
    if not isinstance(ac, MATActorCritic):
        return None, "not a MATActorCritic"
    if pol.action_dtype != "discrete":
        return None, "the fused MAT update covers Discrete actions"
    D = ac.actor.embedding_size
    if D != 64 or ac.critic.embedding_size != 64:
        return None, f"embedding {D} (the fused kernel is built for 64)"
    if len(ac.actor.blocks) != 1 or len(ac.critic.blocks) != 1:
        return None, "more than one block"
    atts = [ac.actor.blocks[0].attn1, ac.actor.blocks[0].attn2, ac.critic.blocks[0].attn]
    if any(a.num_heads != 1 for a in atts):
        return None, "more than one attention head"
    gelus = [m for m in ac.modules() if isinstance(m, nn.GELU)]
    others = [m for m in ac.modules() if isinstance(m, (nn.ReLU, nn.Tanh, nn.LeakyReLU, nn.Sigmoid, nn.ELU))]
    if others or any(getattr(m, "approximate", "none") != "none" for m in gelus):
        return None, "activations other than exact GELU"
    named = list(ac.named_parameters())
    if [n for n, _ in named] != _MAT_PARAM_NAMES:
        return None, "parameter list differs from the default MATActorCritic"
    NA, O, A = ac.actor.action_pred_size, ac.critic.in_size, ac.actor.num_agents
    if not (1 <= NA <= 8 and 1 <= O <= MAT_MAX_OBS and 1 <= A <= 16):
        return None, f"sizes (actions {NA}, obs {O}, agents {A}) outside the fused kernel's limits (8, {MAT_MAX_OBS}, 16)"
    if ac.actor.action_encoder[0].in_features != NA + 1 or ac.actor.action_encoder[0].bias is not None:
        return None, "action encoder is not the Discrete (start token + one-hot, no bias) form"
    base = ac.flat_params.data_ptr()
    offs, off = [], 0
    for _, p in named:
        if (p.data_ptr() - base) // 4 != off:
            return None, "parameter layout differs from the kernel's table"
        offs.append(off)
        off += (p.numel() + 3) // 4 * 4
    if off != ac.flat_params.numel():
        return None, "bucket holds parameters the fused kernel does not know about"
    return dict(obs_dim=O, num_agents=A, num_actions=NA, embedding=64, offsets=offs, bucket_total=off), ""


class FusedMatUpdate(FusedEpoch):
    """
    Host driver of K15 (csrc/mat_update.hip).  Same epoch protocol as FusedPolicyUpdate: records of
    every mini-batch up front, then per mini-batch fwd_bwd -> reduce -> [all-reduce] -> K11 clip + Adam,
    `graph_chunk` mini-batches per hipGraph on a single rank.
    """

    @staticmethod
    def unsupported_reason(pol, batch_size):
        if not pol.agent_grouping:
            return "not an agent-grouped policy"
        _, why = _describe_mat(pol)
        if not why and batch_size < 2:
            return "batch size < 2"
        return why

    def __init__(self, ppo, policy_id):
        super().__init__(ppo, policy_id)
        pol = self.pol
        dev = pol.device
        self.topo, _ = _describe_mat(pol)
        self.per_tile = 16 // self.topo["num_agents"]
        self.n_wg = (self.B + self.per_tile - 1) // self.per_tile
        total = self.topo["bucket_total"]
        self.slabs = torch.zeros(self.n_wg, total, dtype=torch.float32, device=dev)
        _init_normaliser(self)
        self.loss_partials = torch.zeros(self.n_wg, 8, dtype=torch.float32, device=dev)
        self._open_exchange(total)
        # split-wgrad chain (csrc/mat_update.hip: mat_update_wgrad_kernel): PPOAF_SPLIT_WGRAD = auto (= 1) | 1 | 0.  The reduce
        # entry point keeps its contract (slabs / panels -> gradient bucket), so every path above it -- graphs, K17, the
        # RCCL loops -- is the same with either form.
        self.split = split_wgrad_mode() != "0"
        self._norm_partials = {}

    def _make_args(self, B):
        pol, ppo, buf = self.pol, self.ppo, self.pol.buffer
        a = _lib.MatUpdateArgs()
        t = self.topo
        a.obs_dim, a.num_agents, a.num_actions, a.embedding = t["obs_dim"], t["num_agents"], t["num_actions"], 64
        for i, o in enumerate(t["offsets"]):
            a.offsets[i] = o
        a.bucket_total = t["bucket_total"]
        ac = pol.actor_critic
        a.params, a.grads, a.slabs = ac.flat_params.data_ptr(), ac.flat_grads.data_ptr(), self.slabs.data_ptr()
        a.perm, a.row_map = self.perm.data_ptr(), buf.row_map.data_ptr()
        _loss_args(self, a, B)
        opt = pol.actor_critic_optim
        a.norm_scratch, a.step_count = opt.norm_scratch.data_ptr(), opt.step_count.data_ptr()
        # the reduce launch also advances the step count and yields the local ||g||^2 (replaced by K17's norm of the
        # summed gradient when ranks exchange); only the RCCL path runs the separate K11 norm pass
        a.fuse_norm = int(not self.multi or self.xchg is not None)
        a.split_workspace, a.split_workspace_bytes = None, 0
        if self.split:
            if self._split_space is None:                # sized once, for the full batch size (a tail mini-batch needs less)
                need = C.c_int64(0)
                _lib.check(self._lib.ppoaf_mat_update_split_workspace_bytes(C.byref(a), C.byref(need)), "mat_update_split_workspace_bytes")
                self._split_space = torch.zeros(int(need.value), dtype=torch.uint8, device=pol.device)
            a.split_workspace, a.split_workspace_bytes = self._split_space.data_ptr(), self._split_space.numel()
        n = int(self._lib.ppoaf_mat_update_norm_partials(C.byref(a)))
        if n < 0:
            _lib.check(n, "mat_update_norm_partials")
        self._norm_partials[B] = n
        if opt.norm_scratch.numel() < 2 + n:             # one squared-norm partial per workgroup of the reduce launch
            opt.norm_scratch = torch.zeros(2 + n, dtype=torch.float64, device=pol.device)
            a.norm_scratch = opt.norm_scratch.data_ptr()
        return a

    def _signature(self):
        buf = self.pol.buffer
        return (buf.critic_observations.data_ptr(), self.tables["critic_obs"].data_ptr(), buf.num_transitions,
                self.perm.data_ptr()) + _loss_signature(self)

    @property
    def norm_partials(self):
        """How ppoaf_adam_step_prenormed finds ||g||^2: the reduce launch's per-workgroup partials (single rank), or
        norm_scratch[0] as K17's exchange left it (0)."""
        if self.xchg is not None:
            return 0
        return self._norm_partials.get(self.B) or (self.topo["bucket_total"] // 4 + 255) // 256

    def _chain_allreduce(self, ref, comm, k, st):
        """fwd_bwd -> reduce -> all-reduce -> K11 clip + Adam per mini-batch."""
        pol = self.pol
        opt, clip = pol.actor_critic_optim, pol.gradient_clip
        _lib.check(self._lib.ppoaf_mat_update_chain_allreduce(
            ref, comm, k, opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(), opt.lr.data_ptr(), opt.betas[0], opt.betas[1],
            opt.eps, 1.0 / self.world, float(clip) if clip is not None else 0.0, opt.grad_norm.data_ptr(), st),
            "mat_update_chain_allreduce")

    def _epoch_inputs(self, N):
        pol, ppo, buf = self.pol, self.ppo, self.pol.buffer
        ds = pol.dataset
        self._gather_tables(dict(critic_obs=buf.critic_observations, raw_actions=buf.raw_actions, advantages=buf.advantages,
                                 log_probs=buf.log_probs, rewards_to_go=buf.rewards_to_go))

        def keep(name, rec):
            cur = getattr(self, name)
            if cur is None or cur.shape != rec.shape:
                setattr(self, name, torch.empty_like(rec))
                self._graphs.clear()
            getattr(self, name).copy_(rec)

        if ppo.normalize_values:
            rec = ppo._epoch_records(self.policy_id, ds, self.perm, self.B)             # [R, nb, 3]
            keep("records", rec.permute(1, 0, 2).contiguous())
            _seed_normaliser(self)
        if ppo.normalize_adv:
            keep("adv_records", ppo._epoch_records(self.policy_id, ds, self.perm, self.B, field="advantages",
                                                   gather=False)[0].contiguous())

    # ---- fused tail of K15's split-wgrad chain (csrc/mat_update.hip: mat_update_wgrad_adam_kernel): weight gradients, the
    # clip norm from tagged records and clip + Adam in ONE launch (single rank) -- two launches per mini-batch
    _tail_ctl_bytes = "mat_update_tail_ctl_bytes"
    _waits = (_TAIL_WAIT,)

    def tail_reason(self):
        if _switch("PPOAF_FUSED_TAIL", "1") == "0":
            return "off (PPOAF_FUSED_TAIL=0)"
        if getattr(self, "_tail_disabled", ""):
            return "disabled after a failed launch: " + self._tail_disabled
        if not self.split:
            return "the slab form runs (PPOAF_SPLIT_WGRAD=0)"
        if self.multi:
            return "N > 1: the gradient exchange sits between the weight gradients and the optimiser step"
        return ""

    def _epoch_state(self):
        pol = self.pol
        opt, ac = pol.actor_critic_optim, pol.actor_critic
        return [ac.flat_params, opt.exp_avg, opt.exp_avg_sq, opt.step_count, self.vn_mean, self.vn_var, self.vn_count, pol.buffer.values]

    _chunk = _chunk_with_offsets
    _publish = _publish_normaliser

    def _one(self, args):
        lib, st, ref = self._lib, K.stream(), C.byref(args)
        rc = lib.ppoaf_mat_update_fwd_bwd(ref, st)
        if rc == 0 and self.tail_reason() == "":
            opt, clip = self.pol.actor_critic_optim, self.pol.gradient_clip
            rc = lib.ppoaf_mat_update_wgrad_adam(
                ref, self._tail_ctl_ptr(args), opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(), opt.lr.data_ptr(), opt.betas[0],
                opt.betas[1], opt.eps, 1.0, float(clip) if clip is not None else 0.0, opt.grad_norm.data_ptr(),
                self.tail_wait_seconds, st)
            self._tail_used = True
            if rc != 0:
                _lib.check(rc, "mat_update_wgrad_adam")
            return
        if rc == 0:
            rc = lib.ppoaf_mat_update_reduce(ref, st)
        if rc != 0:
            _lib.check(rc, "mat_update")
        if self.multi and self.xchg is None:
            mpi_utils.allreduce_sum_(self.pol.policy_grads)
            self.pol.optimizer_step(1.0 / self.world)
            return
        opt, ac = self.pol.actor_critic_optim, self.pol.actor_critic
        clip = self.pol.gradient_clip
        if self.xchg is not None:
            self.xchg.allreduce(ac.flat_grads, ac.flat_grads, norm_scale=1.0 / self.world, norm_out=opt.norm_scratch, stream=st)
        rc = lib.ppoaf_adam_step_prenormed(
            ac.flat_params.data_ptr(), ac.flat_grads.data_ptr(), opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(),
            ac.flat_params.numel(), opt.step_count.data_ptr(), opt.lr.data_ptr(), opt.betas[0], opt.betas[1], opt.eps,
            1.0 / self.world, float(clip) if clip is not None else 0.0, opt.norm_scratch.data_ptr(), self.norm_partials,
            opt.grad_norm.data_ptr(), st)
        if rc != 0:
            _lib.check(rc, "adam_step_prenormed")
