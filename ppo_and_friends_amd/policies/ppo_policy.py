"""
PPOPolicy -- the policy surface PPO drives (policies/ppo_policy.py:26-1419 of the
reference), rebuilt on the device-resident rollout buffer and the HIP kernels.

Same constructor keywords, attributes and method names as the reference for the
hot path: register_agent, finalize, initialize_dataset,
initialize_episodes, get_rollout_actions, get_critic_values, add_episode_info,
end_episodes, finalize_dataset, clear_dataset, evaluate, update_weights,
update_learning_rate, get_bs_clip_range, save / load.

What changed underneath
  * episodes are flags in a `[T, A*E]` SoA buffer, not E Python objects
    (utils/episode_info.py here); observations / actions may arrive as numpy
    arrays (reference call shape) or as device tensors (no host round trip);
  * the distribution is evaluated on the device (the reference moves the actor
    output to the CPU: ppo_policy.py:770,930);
  * update_weights = backward -> one RCCL all-reduce of the flat gradient bucket
    -> fused clip + Adam kernels (reference: per-tensor pickled MPI allreduce,
    clip_grad_norm_, Adam.step: ppo_policy.py:1032-1055).
"""
import os

import numpy as np
import torch

from .. import kernels as K
from ..networks.distributions import get_actor_distribution
from ..networks.feed_forward import FeedForwardNetwork
from ..spaces import (get_action_prediction_shape, get_flattened_space_length,
                      get_space_dtype_str, get_space_shape)
from ..utils import mpi_utils
from ..utils.episode_info import PPODataset, RolloutBuffer
from ..utils.mpi_utils import rank_print
from ..utils.schedulers import CallableValue


def _callable(v):
    return v if callable(v) else CallableValue(v)


class FlatAdam:
    """
    Adam(eps=1e-5) + clip_grad_norm_ over a flat bucket (ppo_policy.py:336-343,
    1037-1042) as two HIP launches; step counter and lr live on the device.
    """

    def __init__(self, network, lr, eps=1e-5, betas=(0.9, 0.999), storage=None):
        """storage = (exp_avg, exp_avg_sq, step_count[1], lr[1], norm_scratch or None) views of a policy-wide
        allocation (so the fused update kernels see actor and critic state adjacent).  norm_scratch is this
        optimiser's own float64[2 + partials] (K11's / K15's per-workgroup squared-norm partials)."""
        self.network = network
        dev = network.flat_params.device
        if storage is None:
            storage = (torch.zeros_like(network.flat_params), torch.zeros_like(network.flat_params),
                       torch.zeros(1, dtype=torch.int64, device=dev),
                       torch.full((1,), float(lr), dtype=torch.float32, device=dev), None)
        self.exp_avg, self.exp_avg_sq, self.step_count, self.lr, self.norm_scratch = storage
        if self.norm_scratch is None:
            self.norm_scratch = torch.zeros(max(K.NORM_SCRATCH_DOUBLES, 2 + (network.flat_params.numel() + 1023) // 1024),
                                            dtype=torch.float64, device=dev)
        self.lr.fill_(float(lr))
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.eps = eps
        self.betas = betas
        self.param_groups = [{"lr": float(lr)}]      # torch.optim surface for update_optimizer_lr

    def zero_grad(self):
        self.network.flat_grads.zero_()

    def step(self, grad_scale=1.0, max_norm=None):
        K.clip_adam_step(self.network.flat_params, self.network.flat_grads, self.exp_avg,
                         self.exp_avg_sq, self.step_count, self.lr, self.norm_scratch,
                         beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                         grad_scale=grad_scale, max_norm=max_norm, grad_norm_out=self.grad_norm)

    def set_lr(self, lr):
        self.param_groups[0]["lr"] = float(lr)
        self.lr.fill_(float(lr))

    def state_dict(self):
        """torch.optim.Adam.state_dict() layout (what the reference torch.saves, ppo_policy.py:1239-1247)."""
        from ..utils.reference_io import adam_state_dict
        return adam_state_dict(self.network, self.exp_avg, self.exp_avg_sq, int(self.step_count.item()),
                               self.param_groups[0]["lr"], self.betas, self.eps)

    def load_state_dict(self, sd):
        if "param_groups" in sd:
            from ..utils.reference_io import load_adam_state_dict
            step, lr = load_adam_state_dict(sd, self.network, self.exp_avg, self.exp_avg_sq)
            self.step_count.fill_(step); self.set_lr(lr)
            return
        self.exp_avg.copy_(sd["exp_avg"]); self.exp_avg_sq.copy_(sd["exp_avg_sq"])      # this package's old layout
        self.step_count.fill_(int(sd["step"])); self.set_lr(sd["lr"])


class PPOPolicy:

    fused_icm_reward_calls = 0         # intrinsic-reward calls answered by K14's two launches in this process (tests: the path ran)
    # Opt-in: the agent-shared ICM of an agent-grouped policy (MultiDiscrete over the group, ppo.py:2520-2538) on K14's
    # kernels, update epoch and rollout-time reward.  Set on the policy before its first rollout: it is read when the ICM
    # updater and the reward state are first built.  False: the torch path, with today's messages.
    fused_shared_icm = False
    # Opt-in: a wide pair (256-wide actor, 512-wide critic; `fused_wide_critic`) with 65 .. 128 inputs to either network on
    # K6+K7 and K12: the layer-0 panel of such a network takes a row stride of 128 instead of 64 (the library's
    # PPOAF_SPLIT_WIDE_INPUTS).  Set by hand, on the class or on the policy, before the first rollout -- no update_mode sets it.  False:
    # the torch path for those shapes, with today's messages; at in_dim <= 64 the flag changes nothing, bitwise.
    fused_wide_inputs = False
    # Opt-in, implies `fused_wide_inputs`: the wide pair at in_dim <= 512 per network (as far as each row-tile body's LDS goes:
    # a 256-wide actor of depth 1 / 2 holds 512 inputs, of depth 3 432, of depth 4 160) and batch sizes <= 1024 on K6+K7 and
    # K12 (the library's PPOAF_SPLIT_WIDE_SHAPES: layer-0 panels of stride 256 or 512, the weight-gradient launch in passes of
    # 32 chunks of 16 rows).  Set by hand, on the class or on the policy, before the first rollout -- no update_mode sets it.
    # False: the torch path for those shapes, with today's messages; inside the other opt-in's limits the flag changes nothing, bitwise.
    fused_wide_shapes = False
    # Opt-in: the wide pair's actor with 9 .. 24 outputs under a Categorical or tanh-Gaussian head (Discrete(18), Box(17)) on
    # K6+K7, K12 and K19: kernels of their own, which the library picks from out_dim (fused_update.WIDE_HEAD_MAX).  Set by hand,
    # on the class or on the policy, before the first rollout -- no update_mode sets it; it combines with the two flags above
    # (376 inputs need `fused_wide_shapes`).  False: the torch path for those heads, with today's messages ("output width 17 >
    # 8"); a policy with out_dim <= 8 computes bitwise the same, flag on or off.  MultiDiscrete / MultiBinary heads, LSTM and
    # MAT policies, ICMs and every other width pair keep 8.
    fused_wide_heads = False
    # Opt-in: the wide pair on N > 1 ranks (DD-PPO), at every shape it takes on one rank with the flags above: the three-launch
    # split-wgrad chain with the gradient all-reduce between its wgrad and Adam launches (Adam then runs its own norm pass); from
    # C where the library holds an RCCL communicator (ppoaf_ppo_update_chain_allreduce).  No K17 route yet.  Set by hand, on the class or on the policy,
    # before the first rollout -- no update_mode sets it.  False: on N > 1 ranks the pair is refused with today's message
    # ("single rank only for now"); on one rank the flag changes nothing.
    fused_wide_ranks = False
    # Opt-in: an ICM over Discrete / Box actions of 9 .. 24 classes or dimensions (Discrete(18), Box(17)) on K14's shapes chain
    # and its identity form, update epoch and rollout-time reward: the 32-column action form, which the library runs when
    # the topology carries PPOAF_ICM_WIDE_ACTIONS; a one-width ICM (128/128/128) with such actions goes to the shapes chain too.
    # Set by hand, on the class or on the policy, before the first rollout -- no update_mode sets it.  False: the torch path for
    # those ICMs, with today's messages ("action widths (18, 18) must be in [1, 8]"); an ICM with action widths <= 8 computes
    # bitwise the same, flag on or off.  MultiDiscrete ICMs keep 16 classes in all.
    fused_wide_icm_actions = False

    def __init__(self, name, action_space, actor_observation_space, critic_observation_space,
                 envs_per_proc, bootstrap_clip=(-100., 100.), ac_network=FeedForwardNetwork,
                 actor_kw_args={}, critic_kw_args={}, icm_kw_args={}, target_kl=100.,
                 surr_clip=0.2, vf_clip=None, gradient_clip=0.5, lr=3e-4, icm_lr=3e-4,
                 entropy_weight=0.01, kl_loss_weight=0.0, use_gae=True, gamma=0.99, lambd=0.95,
                 dynamic_bs_clip=False, enable_icm=False, agent_shared_icm=False, icm_network=None,
                 intr_reward_weight=1.0, icm_beta=0.8, use_huber_loss=False, test_mode=False,
                 verbose=False, random_seed=0, **kw_args):
        # ppo_policy.py:164-212
        self.name = name
        self.action_space = action_space
        self.actor_obs_space = actor_observation_space
        self.critic_obs_space = critic_observation_space
        self.enable_icm = enable_icm
        self.agent_shared_icm = agent_shared_icm
        self.test_mode = test_mode
        self.use_gae = use_gae
        self.gamma = gamma
        self.lambd = lambd
        self.dynamic_bs_clip = dynamic_bs_clip
        self.using_lstm = False
        self.dataset = None
        self.buffer = None
        self.device = torch.device("cpu")
        self.agent_ids = np.array([])
        self.icm_beta = icm_beta
        self.target_kl = target_kl
        self.surr_clip = surr_clip
        self.vf_clip = vf_clip
        self.gradient_clip = gradient_clip
        self.kl_loss_weight = kl_loss_weight
        self.envs_per_proc = envs_per_proc
        self.agent_grouping = False
        self.have_step_constraints = False
        self.have_reset_constraints = False
        self.verbose = verbose
        self.use_huber_loss = use_huber_loss
        self.frozen = False
        self.fused_action_heads = False      # MultiDiscrete / MultiBinary heads on K6 / K12 (set by PPO(update_mode="fused"))
        # a 512-wide critic beside a 256-wide actor on K6+K7 / K12 (fused_update.WIDE_WIDTH_PAIRS): set by
        # PPO(update_mode="fused"), or by hand before the first rollout.  False: the torch path, with today's messages.
        self.fused_wide_critic = False
        self.fused_lstm_step = True          # K21 for the rollout / evaluation step of a covered LSTM policy
        self.fused_lstm_update = True        # K22 for the update epoch of a covered LSTM policy (False: the mini-batch loop)
        self.random_seed = random_seed
        self.lr = _callable(lr)
        self.icm_lr = _callable(icm_lr)
        self.entropy_weight = _callable(entropy_weight)
        self.intr_reward_weight = _callable(intr_reward_weight)
        if vf_clip is not None:
            # the reference's vf_clip branch dereferences self.user_huber_loss (ppo.py:2432): unusable there too
            raise NotImplementedError("vf_clip raises AttributeError in the reference (ppo.py:2432); not reproduced")
        self.dynamic_bs_clip = bool(dynamic_bs_clip)

        self.action_dtype = get_space_dtype_str(self.action_space)
        if self.action_dtype not in ("discrete", "continuous", "multi-discrete", "multi-binary"):
            raise NotImplementedError(f"{name}: action dtype {self.action_dtype} is outside the hot-path scope")
        self.have_bootstrap_clip = bootstrap_clip is not None
        self.bootstrap_clip = (None if bootstrap_clip is None
                               else (_callable(bootstrap_clip[0]), _callable(bootstrap_clip[1])))
        self.action_dim = get_flattened_space_length(self.action_space)
        self.action_pred_size = get_action_prediction_shape(self.action_space)[0]
        self.network_args = dict(ac_network=ac_network, enable_icm=enable_icm, icm_network=icm_network,
                                 actor_kw_args=actor_kw_args, critic_kw_args=critic_kw_args,
                                 icm_kw_args=icm_kw_args)
        self.network_args.update(kw_args)
        self._t = 0

    # ------------------------------------------------------------------ setup
    def register_agent(self, agent_id):
        """ppo_policy.py:355-365 (insertion order kept instead of set order: deterministic columns)."""
        if agent_id not in list(self.agent_ids):
            self.agent_ids = np.array(list(self.agent_ids) + [agent_id])

    def finalize(self, status_dict, device):
        """ppo_policy.py:302-345."""
        if len(self.agent_ids) == 0:
            self.register_agent("agent0")
        self.agent_idxs = np.arange(len(self.agent_ids))
        self.num_agents = self.agent_idxs.size
        self._agent_col = {a: i for i, a in enumerate(self.agent_ids)}
        self.device = torch.device(device)
        self._initialize_networks(**self.network_args)
        for c in (self.lr, self.icm_lr, self.entropy_weight, self.intr_reward_weight):
            c.finalize(status_dict)
        if self.have_bootstrap_clip:
            self.bootstrap_clip[0].finalize(status_dict)
            self.bootstrap_clip[1].finalize(status_dict)
        na = self.actor.bucket_size()
        dev = self.device
        self.policy_exp_avg = torch.zeros_like(self.policy_params)
        self.policy_exp_avg_sq = torch.zeros_like(self.policy_params)
        self.policy_step_counts = torch.zeros(2, dtype=torch.int64, device=dev)
        self.policy_lr = torch.full((1,), float(self.lr()), dtype=torch.float32, device=dev)
        # K12: squared norms (2) + Adam bias corrections (4) + per-workgroup squared-norm partials of the bucket
        self.policy_norm_scratch = torch.zeros(6 + 2 * ((self.policy_params.numel() + 1023) // 1024), dtype=torch.float64, device=dev)
        self.actor_optim = FlatAdam(self.actor, self.lr(), eps=1e-5, storage=(
            self.policy_exp_avg[:na], self.policy_exp_avg_sq[:na], self.policy_step_counts[0:1], self.policy_lr, None))
        self.critic_optim = FlatAdam(self.critic, self.lr(), eps=1e-5, storage=(
            self.policy_exp_avg[na:], self.policy_exp_avg_sq[na:], self.policy_step_counts[1:2], self.policy_lr, None))
        self.icm_optim = FlatAdam(self.icm_model, self.icm_lr(), eps=1e-5) if self.enable_icm else None

    def _initialize_networks(self, ac_network, enable_icm, icm_network, actor_kw_args,
                             critic_kw_args, icm_kw_args, **kw_args):
        """ppo_policy.py:390-472: actor out gain 0.01, critic out gain 1.0; rank-0 broadcast."""
        from ..networks.lstm import PPOLSTMNetwork
        self.using_lstm = isinstance(ac_network, type) and issubclass(ac_network, PPOLSTMNetwork)   # ppo_policy.py:420-422
        self.actor = ac_network(name="actor", in_shape=get_space_shape(self.actor_obs_space),
                                out_shape=get_action_prediction_shape(self.action_space),
                                out_init=0.01, test_mode=self.test_mode, **actor_kw_args)
        self.critic = ac_network(name="critic", in_shape=get_space_shape(self.critic_obs_space),
                                 out_shape=(1,), out_init=1.0, test_mode=self.test_mode,
                                 **critic_kw_args)
        self.actor.distribution = get_actor_distribution(
            self.action_space, seed=self.random_seed + 7919 * mpi_utils.get_rank(), **actor_kw_args)
        self._place_networks()
        mpi_utils.broadcast_flat(self.policy_params)      # one message for actor + critic
        if enable_icm:                                    # ppo_policy.py:461-472
            if self.agent_shared_icm:
                raise NotImplementedError("agent_shared_icm needs agent grouping (MAT); not built")
            from ..networks.icm import ICM
            icm_cls = ICM if icm_network is None else icm_network
            self.icm_model = icm_cls(name="icm", obs_space=self.actor_obs_space,
                                     action_space=self.action_space, test_mode=self.test_mode,
                                     **icm_kw_args)
            self.icm_model.to(self.device)
            mpi_utils.broadcast_model_parameters(self.icm_model)

    def seed(self, seed):
        self.random_seed = seed
        self.actor.distribution.rng.seed = int(seed) + 7919 * mpi_utils.get_rank()

    def _place_networks(self):
        """Actor and critic buckets adjacent in one allocation: one broadcast, one all-reduce."""
        na, nc = self.actor.bucket_size(), self.critic.bucket_size()
        self.policy_params = torch.zeros(na + nc, dtype=torch.float32, device=self.device)
        self.policy_grads = torch.zeros(na + nc, dtype=torch.float32, device=self.device)
        self.actor.flatten_parameters_(self.device, (self.policy_params[:na], self.policy_grads[:na]))
        self.critic.flatten_parameters_(self.device, (self.policy_params[na:], self.policy_grads[na:]))

    def to(self, device):
        self.device = torch.device(device)
        self._place_networks()

    def eval(self):
        self.actor.eval(); self.critic.eval()

    def train(self):
        self.actor.train(); self.critic.train()

    def freeze(self):
        self.frozen = True

    def unfreeze(self):
        self.frozen = False

    def shuffle_agent_ids(self):
        np.random.shuffle(self.agent_idxs)
        self.agent_ids = self.agent_ids[self.agent_idxs]

    # ---------------------------------------------------------------- rollout
    def initialize_dataset(self):
        """ppo_policy.py:506-526."""
        sequence_length = 1
        if self.using_lstm:
            self.actor.reset_hidden_state(batch_size=1, device=self.device)
            self.critic.reset_hidden_state(batch_size=1, device=self.device)
            sequence_length = self.actor.sequence_length
        self.dataset = PPODataset(device=self.device, action_dtype=self.action_dtype,
                                  sequence_length=sequence_length)

    def initialize_episodes(self, env_batch_size, status_dict, ts_per_rollout=None):
        """
        ppo_policy.py:474-504.  The reference allocates E EpisodeInfo objects per
        agent; here one `[T, A*E]` buffer.  T = timesteps per env in this rollout
        (ts_per_rollout / envs_per_proc, ppo.py:317-318,1646-1653).
        """
        if ts_per_rollout is None:
            ts_per_rollout = status_dict["global status"]["ts per rollout"] if status_dict else None
        if ts_per_rollout is None:
            raise ValueError("initialize_episodes needs ts_per_rollout (total steps over all envs)")
        T = int(ts_per_rollout) // int(env_batch_size)
        self.env_batch_size = int(env_batch_size)
        C = self.env_batch_size * len(self.agent_ids)
        obs_dim = int(np.prod(get_space_shape(self.actor_obs_space)))
        cobs_dim = int(np.prod(get_space_shape(self.critic_obs_space)))
        if self.buffer is None or (self.buffer.T, self.buffer.C) != (T, C):
            lstm_spec = None
            if self.using_lstm:
                lstm_spec = ((self.actor.num_lstm_layers, self.actor.lstm_hidden_size),
                             (self.critic.num_lstm_layers, self.critic.lstm_hidden_size))
            self.buffer = RolloutBuffer(T, C, obs_dim, cobs_dim, self.action_dim, self.action_dtype,
                                        self.device, keep_next_observations=self.enable_icm, lstm_spec=lstm_spec)
        else:
            self.buffer.end_kind.zero_()
            self.buffer.fixed_length = True
            self.buffer.steps_written = 0
        self._t = 0
        self._agents_written = 0
        self.dataset.attach(self.buffer, self.gamma, self.lambd, self.get_bs_clip_range(None), self.use_gae)

    def _to_device(self, x, dtype=torch.float32):
        if torch.is_tensor(x):
            return x.to(device=self.device, dtype=dtype)
        return torch.as_tensor(np.asarray(x), dtype=dtype).to(self.device)

    def get_rollout_actions(self, obs, forced_raw_action=None):
        """
        ppo_policy.py:729-794 -> (raw_action, action, log_prob).  numpy in -> numpy
        actions out (reference contract); device tensor in -> device tensors out.
        forced_raw_action: recorded raw actions to log instead of sampling (replay of a rollout).
        """
        if len(obs.shape) < 2:
            raise ValueError(f"get_rollout_actions expects a batch of observations, got shape {obs.shape}")
        as_numpy = not torch.is_tensor(obs)
        t_obs = self._to_device(obs)
        with torch.no_grad():
            pred = self.actor.forward_logits(t_obs)
            if forced_raw_action is None:
                action, raw_action, log_prob = self.actor.distribution.sample_distribution(pred)
            else:
                dist = self.actor.distribution
                raw_action = self._to_device(forced_raw_action, torch.float32 if self.action_dtype == "continuous" else torch.int64)
                raw_action = raw_action.reshape(pred.shape[0], -1)
                log_prob, _ = dist.get_log_probs_and_entropy(pred, raw_action)
                action = dist.refine_prediction(raw_action) if self.action_dtype == "continuous" else raw_action
        if as_numpy:
            return raw_action.cpu().numpy(), action.cpu().numpy(), log_prob.detach()
        return raw_action, action, log_prob

    # ---- LSTM hidden states (ppo_policy.py:593-627, ppo.py:2312-2319,2450-2466)
    def store_hidden_states(self, t, terminated):
        """
        Row t of the buffer receives the networks' (hidden, cell) AFTER this step's forward passes,
        zeroed for the envs that terminated at this step.  The networks' own state is NOT reset
        (the reference never resets it inside a rollout).
        """
        keep = (~terminated).to(torch.float32).view(-1, 1, 1)
        h = self.buffer.hidden
        for name, net in (("actor", self.actor), ("critic", self.critic)):
            hid, cell = net.hidden_state                       # [layers, C, H]
            h[name + "_hidden"][t].copy_(hid.transpose(0, 1) * keep)
            h[name + "_cell"][t].copy_(cell.transpose(0, 1) * keep)

    def load_hidden_states(self, mb):
        """ppo.py:2312-2319: the mini-batch's stored states become the networks' initial states."""
        self.actor.hidden_state = (mb["actor_hidden"].transpose(0, 1).contiguous(),
                                   mb["actor_cell"].transpose(0, 1).contiguous())
        self.critic.hidden_state = (mb["critic_hidden"].transpose(0, 1).contiguous(),
                                    mb["critic_cell"].transpose(0, 1).contiguous())

    def write_back_hidden_states(self, dataset, batch_idxs):
        """ppo.py:2450-2466: the states the networks ended the window with replace the stored ones."""
        dataset.actor_hidden[batch_idxs] = self.actor.hidden_state[0].detach().transpose(0, 1)
        dataset.critic_hidden[batch_idxs] = self.critic.hidden_state[0].detach().transpose(0, 1)
        dataset.actor_cell[batch_idxs] = self.actor.hidden_state[1].detach().transpose(0, 1)
        dataset.critic_cell[batch_idxs] = self.critic.hidden_state[1].detach().transpose(0, 1)

    def fused_step_unsupported_reason(self):
        """'' when the K6+K7 rollout-step kernel covers this policy (same coverage as the fused update)."""
        from ..fused_update import FusedPolicyUpdate
        return FusedPolicyUpdate.unsupported_reason(self, 2)

    def rollout_step(self, t, obs, critic_obs, value_normalizer=None, forced_raw_action=None, blocks=None):
        """
        blocks (optional, then obs / critic_obs are None): (obs_blocks, critic_obs_blocks, env_action_blocks), one
        device tensor per agent of the policy in env order -- [E_env, .] float32 rows of the env's observation tensors
        where they lie (slices of an agent-major tensor or a dict env's entries) and the env's action tensors, which the
        launch fills beside the buffer row (ppoaf_policy_step_blocks); `step_blocks_unsupported_reason` says when not.
        forced_raw_action (optional contiguous device tensor shaped like the step's raw actions: [E] / [E,1] int64
        (Discrete), [E,D] int64 (MultiDiscrete, one class per slice), [E,D] float32 (Box) or [E,n] float32 of 0 / 1
        (MultiBinary)): log these raw actions instead of sampling -- replay of a recorded rollout (log-probs, refined actions and values are computed
        as usual).
        One env step of get_rollout_actions + get_critic_values (+ denormalisation) +
        add_episode_info's action/value/log-prob/observation writes, as ONE launch that
        stores straight into row t of the rollout buffer.  Returns the action row (a
        view of the buffer) for env.step; rewards / next observations are added by
        `finish_step` once the environment has answered.
        """
        from .. import _lib
        from ..fused_update import describe_policy, set_head_args
        buf = self.buffer
        E = buf.C                       # agents x envs rows, agent-major
        a = getattr(self, "_step_args", None)
        if a is None:
            a = _lib.PolicyStepArgs()
            desc, _ = describe_policy(self)     # (a covered policy: the callers have asked fused_step_unsupported_reason)
            a.actor, a.critic = desc.actor, desc.critic
            a.params = self.policy_params.data_ptr()
            a.E = E
            set_head_args(a, desc, self.actor.distribution)
            self._step_args = a
        if blocks is None:
            K._req(obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous() and obs.numel() == E * a.actor.in_dim,
                   "rollout_step: obs must be a contiguous float32 device tensor [E, obs_dim]")
            K._req(critic_obs.is_cuda and critic_obs.dtype == torch.float32 and critic_obs.is_contiguous()
                   and critic_obs.numel() == E * a.critic.in_dim,
                   "rollout_step: critic_obs must be a contiguous float32 device tensor [E, critic_obs_dim]")
            a.obs = obs.data_ptr(); a.critic_obs = critic_obs.data_ptr()
        else:
            why = self.step_blocks_unsupported_reason(*blocks)
            if why:
                raise _lib.PpoafError(f"rollout_step: {why}")
            tb = getattr(self, "_step_blocks", None)
            if tb is None:
                tb = self._step_blocks = _lib.StepBlocks()
            tb.n_blocks, tb.rows_per_block = len(blocks[0]), E // len(blocks[0])
            for b, (o, co, ea) in enumerate(zip(*blocks)):
                tb.obs[b], tb.critic_obs[b], tb.env_action[b] = o.data_ptr(), co.data_ptr(), ea.data_ptr()
            a.obs = a.critic_obs = None
        a.forced_raw_action = None
        if forced_raw_action is not None:
            want = torch.float32 if a.head_kind in (K.HEAD_GAUSSIAN, K.HEAD_BERNOULLI) else torch.int64
            K._req(forced_raw_action.is_cuda and forced_raw_action.dtype == want and forced_raw_action.is_contiguous()
                   and forced_raw_action.numel() == buf.raw_actions[t].numel(),
                   "rollout_step: forced_raw_action must be a contiguous device tensor shaped like the step's raw actions")
            a.forced_raw_action = forced_raw_action.data_ptr()
        # Philox counters as the torch path takes them: one per row, one per (slice, row) for MultiDiscrete (slice j of
        # row e draws offset + j * E + e), one per (row, bit) for MultiBinary
        per_row = {K.HEAD_MULTI_CATEGORICAL: a.n_action_slices, K.HEAD_BERNOULLI: a.actor.out_dim}.get(a.head_kind, 1)
        a.seed, a.offset = self.actor.distribution.rng.take(E * per_row)
        if value_normalizer is not None:
            a.normalize_values = 1
            a.vn_mean = value_normalizer.running_stats.mean_t.data_ptr()
            a.vn_var = value_normalizer.running_stats.var_t.data_ptr()
        else:
            a.normalize_values = 0
        a.raw_action_out = buf.raw_actions[t].data_ptr(); a.action_out = buf.actions[t].data_ptr()
        a.logp_out = buf.log_probs[t].data_ptr(); a.value_out = buf.values[t].data_ptr()
        a.obs_copy_out = buf.observations[t].data_ptr()
        a.critic_obs_copy_out = buf.critic_observations[t].data_ptr()
        if blocks is None:
            K.policy_step(a)
        else:
            K.policy_step_blocks(a, tb)
        return buf.actions[t]

    def step_blocks_unsupported_reason(self, obs_blocks, critic_obs_blocks, env_action_blocks):
        """'' when ppoaf_policy_step_blocks takes these row blocks (the library checks the same before it launches)."""
        from .. import _lib
        buf = self.buffer
        n = len(obs_blocks)
        if not 1 <= n <= _lib.ROW_BLOCKS_MAX:
            return f"{n} row blocks, a table holds 1 .. {_lib.ROW_BLOCKS_MAX}"
        if len(critic_obs_blocks) != n or len(env_action_blocks) != n or buf.C % n:
            return f"{n} observation blocks, {len(critic_obs_blocks)} critic and {len(env_action_blocks)} action blocks for {buf.C} rows"
        rows = buf.C // n
        adt, per_row = buf.actions.dtype, buf.actions[0].numel() // buf.C
        for what, blks, dt, width in (("observation", obs_blocks, torch.float32, buf.observations.shape[-1]),
                                      ("critic observation", critic_obs_blocks, torch.float32, buf.critic_observations.shape[-1]),
                                      ("env action", env_action_blocks, adt, per_row)):
            for b, x in enumerate(blks):
                if not (torch.is_tensor(x) and x.is_cuda and x.dtype == dt and x.is_contiguous() and x.numel() == rows * width):
                    return f"{what} block {b} is not a contiguous {dt} device tensor of {rows} x {width}"
                if x.data_ptr() % 16:
                    return f"{what} block {b} does not start on a 16-byte boundary"
        return ""

    # ---- K21: the rollout / evaluation step of an LSTM policy in one launch (csrc/lstm_policy_step.hip)
    def lstm_step_unsupported_reason(self):
        """'' when K21 (ppoaf_lstm_policy_step) covers this policy: a device LSTM policy that PPO has not put on the
        torch path, both networks on K18 (`use_hip`) with one LSTM hidden size, and the library's own check accepting;
        else why today's route (forward_logits + torch ops) is taken.  `fused_lstm_step = False` switches K21 off."""
        if not self.using_lstm:
            return "not an LSTM policy"
        if not getattr(self, "fused_lstm_step", True):
            return "fused_lstm_step is switched off on this policy"
        if self.device.type != "cuda":
            return f"the policy lives on {self.device}: K21 needs a HIP device"
        if getattr(self, "update_mode", "auto") == "torch":
            return "update_mode='torch' keeps the policy on the torch-ROCm path"
        key = (self.policy_params.data_ptr(), bool(self.actor.use_hip), bool(self.critic.use_hip), bool(self.enable_icm))
        if getattr(self, "_lstm_step_reason", (None, ""))[0] != key:
            self._lstm_step_reason = (key, self._lstm_step_scope())
        return self._lstm_step_reason[1]

    def _lstm_step_scope(self):
        from ..fused_update import FusedLstm
        why = FusedLstm.unsupported_reason(self)
        if why:
            return why
        if not (self.actor.use_hip and self.critic.use_hip):
            return "the networks run nn.LSTM (use_hip is not set: update_mode='auto' keeps today's route)"
        ha, hc = self.actor.lstm_hidden_size, self.critic.lstm_hidden_size
        if ha != hc:
            return f"LSTM hidden sizes differ (actor {ha}, critic {hc}): one K21 launch has one block size"
        if self.enable_icm:
            return "ICM policies keep today's route (K21 does not keep the next-observation rows)"
        # what the library itself refuses: host only, nothing is launched and no pointer is followed
        a = self._new_lstm_step_args(1)
        a.mode, a.infer_mode = K.LSTM_INFER, K.INFER_DETERMINISTIC
        a.obs = a.actor_h = a.actor_c = a.action_out = self.policy_params.data_ptr()
        return K.lstm_policy_step_refusal(a)

    def _new_lstm_step_args(self, E):
        """_lib.LstmPolicyStepArgs with everything that stays from step to step, for E rows."""
        from .. import _lib
        from ..fused_update import _activation_code
        from ..networks.distributions import GaussianDistribution
        a = _lib.LstmPolicyStepArgs()
        for tag, net in (("actor", self.actor), ("critic", self.critic)):
            d = getattr(a, tag)
            dims = net.ff_layers.layer_dims()
            d.in_dim, d.hidden, d.ff_hidden, d.ff_depth = net.in_size, net.lstm_hidden_size, dims[0][1], len(dims) - 1
            d.out_dim, d.activation = net.out_size, _activation_code(net.activation)
            d.rows, d.steps = E, 1
            d.params = net.flat_params.data_ptr()
        a.E = E
        dist = self.actor.distribution
        gauss = isinstance(dist, GaussianDistribution)
        a.head_kind = K.HEAD_GAUSSIAN if gauss else K.HEAD_CATEGORICAL
        a.min_std = float(getattr(dist, "min_std", 0.01))
        if gauss:
            a.log_std = dist.log_std.data_ptr()
            lo, hi = dist.bound_tensors()
            a.act_lo = None if lo is None else lo.data_ptr()
            a.act_hi = None if hi is None else hi.data_ptr()
        return a

    def _lstm_step_args(self, E):
        """The K21 arguments for E rows, and both networks' (h, c) as its in / out buffers: reset by the networks' own
        rule (lstm.py:109-113: when the batch size changes), then stepped in place."""
        st = getattr(self, "_lstm_step_state", None)
        key = (E, self.policy_params.data_ptr())
        if st is None or st["key"] != key:
            st = self._lstm_step_state = dict(key=key, args=self._new_lstm_step_args(E),
                                              one=torch.ones(1, dtype=torch.uint8, device=self.device))
        for net in (self.actor, self.critic):
            hs = net.hidden_state
            if hs is None or hs[0].shape[1] != E:
                net.reset_hidden_state(batch_size=E, device=self.device)
            elif not (hs[0].is_contiguous() and hs[1].is_contiguous()):
                net.hidden_state = (hs[0].contiguous(), hs[1].contiguous())
        return st

    def _lstm_stored_rows(self, t):
        h = self.buffer.hidden
        return h["actor_hidden"][t], h["actor_cell"][t], h["critic_hidden"][t], h["critic_cell"][t]

    def lstm_step_blocks_unsupported_reason(self, obs_blocks, critic_obs_blocks, env_action_blocks):
        """'' when ppoaf_lstm_policy_step_blocks takes these row blocks: one device tensor per agent of the policy in env
        order, [E_env, .] rows of the env's tensors where they lie.  obs_blocks and env_action_blocks are None for the
        critic's step on the next observation (CRITIC_NEXT reads the critic's blocks only).  The loads are scalar, so a
        block needs its element's alignment only; the library checks the same before it launches."""
        from .. import _lib
        buf = self.buffer
        n = len(critic_obs_blocks)
        if not 1 <= n <= _lib.ROW_BLOCKS_MAX:
            return f"{n} row blocks, a table holds 1 .. {_lib.ROW_BLOCKS_MAX}"
        if buf.C % n or any(b is not None and len(b) != n for b in (obs_blocks, env_action_blocks)):
            return f"{n} critic observation blocks do not pair with the other blocks or with {buf.C} rows"
        rows = buf.C // n
        adt, per_row = buf.actions.dtype, buf.actions[0].numel() // buf.C
        for what, blks, dt, width in (("observation", obs_blocks, torch.float32, buf.observations.shape[-1]),
                                      ("critic observation", critic_obs_blocks, torch.float32, buf.critic_observations.shape[-1]),
                                      ("env action", env_action_blocks, adt, per_row)):
            for b, x in enumerate(blks or ()):
                if not (torch.is_tensor(x) and x.is_cuda and x.dtype == dt and x.is_contiguous() and x.numel() == rows * width):
                    return f"{what} block {b} is not a contiguous {dt} device tensor of {rows} x {width}"
                if x.data_ptr() % x.element_size():
                    return f"{what} block {b} does not start on a {x.element_size()}-byte boundary"
        return ""

    def _lstm_step_blocks(self, obs_blocks, critic_obs_blocks, env_action_blocks):
        """The checked blocks as the table of ppoaf_lstm_policy_step_blocks (one reusable _lib.LstmStepBlocks)."""
        from .. import _lib
        why = self.lstm_step_blocks_unsupported_reason(obs_blocks, critic_obs_blocks, env_action_blocks)
        if why:
            raise _lib.PpoafError(f"lstm_policy_step_blocks: {why}")
        tb = getattr(self, "_lstm_blocks_table", None)
        if tb is None:
            tb = self._lstm_blocks_table = _lib.LstmStepBlocks()
        n = len(critic_obs_blocks)
        tb.n_blocks, tb.rows_per_block = n, self.buffer.C // n
        for b in range(n):
            tb.critic_obs[b] = critic_obs_blocks[b].data_ptr()
            tb.obs[b] = None if obs_blocks is None else obs_blocks[b].data_ptr()
            tb.env_action[b] = None if env_action_blocks is None else env_action_blocks[b].data_ptr()
        return tb

    def lstm_rollout_step(self, t, obs, critic_obs, value_normalizer=None, forced_raw_action=None, blocks=None):
        """
        rollout_step for an LSTM policy (K21, STEP): both networks' forward passes, sampling (or the forced raw action),
        log-prob, value (+ denormalisation) and row t of the buffer -- actions, log-probs, values, observation copies and
        the four hidden-state rows -- in ONE launch that steps the networks' `hidden_state` tensors in place.  Returns
        the action row for env.step; `lstm_finish_step` takes the environment's answer.
        blocks (optional, then obs / critic_obs are None): (obs_blocks, critic_obs_blocks, env_action_blocks) as for
        `rollout_step` -- the launch reads the env's tensors where they lie and fills the env's action tensors beside
        the buffer row (ppoaf_lstm_policy_step_blocks); `lstm_step_blocks_unsupported_reason` says when not.
        """
        buf = self.buffer
        E = buf.C
        a = self._lstm_step_args(E)["args"]
        tb = None if blocks is None else self._lstm_step_blocks(*blocks)
        a.seed, a.offset = self.actor.distribution.rng.take(E)
        self._lstm_normalizer(a, value_normalizer)
        K.lstm_policy_step(a, obs, critic_obs, self.actor.hidden_state, self.critic.hidden_state, buf.raw_actions[t],
                           buf.actions[t], buf.log_probs[t], buf.values[t], self._lstm_stored_rows(t),
                           buf.observations[t], buf.critic_observations[t], forced_raw_action, blocks=tb)
        return buf.actions[t]

    @staticmethod
    def _lstm_normalizer(a, value_normalizer):
        a.normalize_values = 0
        if value_normalizer is not None:
            a.normalize_values = 1
            a.vn_mean = value_normalizer.running_stats.mean_t.data_ptr()
            a.vn_var = value_normalizer.running_stats.var_t.data_ptr()

    def lstm_finish_step(self, t, rewards, terminated, next_critic_obs=None, cut=None, value_normalizer=None,
                         next_critic_blocks=None):
        """
        The environment's answer for step t of an LSTM policy: rewards (None: K23 has written the row already), and the
        stored hidden rows of the envs that terminated zeroed (ppo_policy.py:593-627).  With `next_critic_obs` the same
        launch (K21, CRITIC_NEXT) writes V(next critic observation) to boot_value[t] and keeps the critic's stepped state
        only where the device flag `cut` (one bool / byte, never read by the host) is set (ppo.py:1863-1881); without it
        the zeroing is a launch of its own (MASK).  `terminated`: one flag per buffer row.  next_critic_blocks instead of
        next_critic_obs: the next critic observation as row blocks (see lstm_rollout_step), and then `terminated` holds
        the per-env flags, one per row of a block.
        """
        buf = self.buffer
        if rewards is not None:
            buf.rewards[t].copy_(rewards.reshape(-1))
        buf.steps_written = max(buf.steps_written, t + 1)
        self._t = t + 1
        a = self._lstm_step_args(buf.C)["args"]
        terminated = terminated.reshape(-1).contiguous()
        if next_critic_obs is None and next_critic_blocks is None:
            K.lstm_mask_stored(a, terminated, self._lstm_stored_rows(t))
            return
        tb = None if next_critic_blocks is None else self._lstm_step_blocks(None, next_critic_blocks, None)
        self._lstm_normalizer(a, value_normalizer)
        K.lstm_critic_next(a, next_critic_obs, self.critic.hidden_state, buf.boot_value[t], cut.reshape(1), terminated,
                           self._lstm_stored_rows(t), blocks=tb)

    def lstm_last_value(self, t, critic_obs, value_normalizer=None, critic_blocks=None):
        """V(critic_obs) after the last step of a rollout -> boot_value[t] (K21, CRITIC_NEXT with the flag set: the critic
        is stepped, as get_critic_values steps it).  Returns that row.  critic_blocks instead of critic_obs: the
        observation as row blocks."""
        buf = self.buffer
        st = self._lstm_step_args(buf.C)
        tb = None if critic_blocks is None else self._lstm_step_blocks(None, critic_blocks, None)
        self._lstm_normalizer(st["args"], value_normalizer)
        K.lstm_critic_next(st["args"], critic_obs, self.critic.hidden_state, buf.boot_value[t], st["one"], blocks=tb)
        return buf.boot_value[t]

    def _lstm_infer_step(self, t_obs, deterministic):
        """K21, INFER: one launch steps the actor's hidden state in place and writes the env action into a reusable
        tensor (K19's shapes and dtypes)."""
        E = t_obs.shape[0]
        hs = self.actor.hidden_state
        if hs is None or hs[0].shape[1] != E:
            self.actor.reset_hidden_state(batch_size=E, device=self.device)
        elif not (hs[0].is_contiguous() and hs[1].is_contiguous()):
            self.actor.hidden_state = (hs[0].contiguous(), hs[1].contiguous())
        st = getattr(self, "_lstm_infer_state", None)
        key = (E, self.policy_params.data_ptr())
        if st is None or st["key"] != key:
            a = self._new_lstm_step_args(E)
            gauss = a.head_kind == K.HEAD_GAUSSIAN
            out = torch.zeros((E, a.actor.out_dim) if gauss else (E,), dtype=torch.float32 if gauss else torch.int64,
                              device=self.device)
            st = self._lstm_infer_state = dict(key=key, args=a, out=out)
        a = st["args"]
        if not deterministic:
            a.seed, a.offset = self.eval_rng().take(E)
        K.lstm_policy_infer(a, t_obs.reshape(E, -1).contiguous(), self.actor.hidden_state, st["out"], deterministic)
        return st["out"]

    def finish_step(self, t, rewards, next_obs=None):
        """The environment's answer for step t: rewards (None: K23 has written the row already) and next observations
        when ICM keeps them."""
        buf = self.buffer
        if rewards is not None:
            buf.rewards[t].copy_(rewards.reshape(-1))
        if buf.next_observations is not None and next_obs is not None:
            buf.next_observations[t].copy_(next_obs.reshape(buf.next_observations[t].shape))
        buf.steps_written = max(buf.steps_written, t + 1)
        self._t = t + 1

    def get_intrinsic_reward(self, prev_obs, obs, action):
        """ppo_policy.py:954-1007: ICM forward without gradients -> intrinsic reward [n] (already weighted)."""
        if len(obs.shape) < 2:
            raise ValueError(f"get_intrinsic_reward expects a batch of observations, got shape {obs.shape}")
        obs_1 = self._to_device(prev_obs)
        obs_2 = self._to_device(obs)
        adt = torch.int64 if self.action_dtype in ("discrete", "multi-discrete") else torch.float32
        act = self._to_device(action, adt)
        if act.dim() != 2:
            act = act.unsqueeze(1)
        if obs_1.is_cuda and getattr(self, "fused_icm_reward", True):
            fused = self._fused_intrinsic_reward(obs_1, obs_2, act)
            if fused is not None:
                return fused
        with torch.no_grad():
            intr, _, _ = self.icm_model(obs_1, obs_2, act)
        return intr.reshape(-1) * float(self.intr_reward_weight())

    def _fused_intrinsic_reward(self, obs_1, obs_2, act):
        """K14's encoder + forward-model kernels on the env batch (two launches; one for an identity encoder); None when not
        covered.  The rows of an agent-shared ICM (one per env, MultiDiscrete classes [n, agents]; MATPolicy) are described
        with the ICM's own action dtype: fused_update.describe_policy_icm."""
        import ctypes as C
        from .. import _lib
        from .. import kernels as K
        st = getattr(self, "_icm_reward_state", None)
        n = obs_1.shape[0]
        if st is None or st["n"] != n:
            from ..fused_update import describe_policy_icm, icm_scratch_floats, icm_topology_args
            topo, why = describe_policy_icm(self)
            if topo is None:
                self.fused_icm_reward = False
                return None
            a = icm_topology_args(topo)
            scratch = torch.zeros(icm_scratch_floats(topo, n)[0], dtype=torch.float32, device=self.device)
            a.params = self.icm_model.flat_params.data_ptr()
            a.act_scratch = scratch.data_ptr()
            a.B, a.batch_stride, a.n_rows, a.fused_adam = n, n, n, 0
            # an ICM with widths of its own (csrc/icm_update_shapes.hip) has entry points of its own
            entry = "ppoaf_icm_shapes_intrinsic_reward" if topo.get("general") else "ppoaf_icm_intrinsic_reward"
            st = self._icm_reward_state = dict(n=n, args=a, scratch=scratch, entry=entry)
        a = st["args"]
        obs_1, obs_2, act = obs_1.reshape(n, -1).contiguous(), obs_2.reshape(n, -1).contiguous(), act.contiguous()
        a.obs, a.next_obs, a.actions = obs_1.data_ptr(), obs_2.data_ptr(), act.data_ptr()
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        scale = float(self.intr_reward_weight()) * float(self.icm_model.reward_scale) / 2.0
        _lib.check(getattr(_lib.load(), st["entry"])(C.byref(a), scale, out.data_ptr(), K.stream()), st["entry"][6:])
        PPOPolicy.fused_icm_reward_calls += 1
        return out

    def inference_unsupported_reason(self):
        """'' when get_inference_actions runs on K19 (ppoaf_policy_infer: the coverage of the K6 rollout step, on a
        device policy that PPO has not put on the torch path), else why the torch path is taken."""
        if self.device.type != "cuda":
            return f"the policy lives on {self.device}: K19 needs a HIP device"
        if getattr(self, "update_mode", "auto") == "torch":
            return "update_mode='torch' keeps the policy on the torch-ROCm path"
        if self.using_lstm:
            return "LSTM policies are not K19's: K21 or forward_logits (see lstm_step_unsupported_reason)"
        # (asked once per evaluation step: the answer is kept for as long as what it depends on stays)
        from ..fused_update import FusedOptIns
        key = (self.policy_params.data_ptr(), FusedOptIns.of(self))
        if getattr(self, "_infer_reason", (None, ""))[0] != key:
            self._infer_reason = (key, self.fused_step_unsupported_reason())
        return self._infer_reason[1]

    def eval_rng(self):
        """The evaluation's Philox stream (seeded from the policy seed and a fixed tag): sampled evaluation never draws
        from distribution.rng, so evaluating does not move the training rollout's random stream."""
        dist = self.actor.distribution
        if getattr(dist, "eval_rng", None) is None:
            from ..networks.distributions import _PhiloxStream
            dist.eval_rng = _PhiloxStream((int(dist.rng.seed) ^ 0x6576616C5F726E67) & 0xFFFFFFFFFFFFFFFF)    # "eval_rng"
        return dist.eval_rng

    def _infer_step(self, t_obs, deterministic):
        """K19: one launch, actor forward -> head -> env action, into a reusable output tensor."""
        from .. import _lib
        from ..fused_update import describe_policy, set_head_args
        E = t_obs.shape[0]
        st = getattr(self, "_infer_state", None)
        if st is None or st["E"] != E or st["params"] != self.policy_params.data_ptr():
            a = _lib.PolicyInferArgs()
            desc, _ = describe_policy(self)     # (a covered policy: get_inference_actions has asked inference_unsupported_reason)
            head, a.actor = desc.head, desc.actor
            a.params = self.policy_params.data_ptr()
            a.E = E
            set_head_args(a, desc, self.actor.distribution)
            shape = {K.HEAD_CATEGORICAL: (E,), K.HEAD_MULTI_CATEGORICAL: (E, len(desc.slices))}.get(head, (E, a.actor.out_dim))
            out = torch.zeros(shape, dtype=torch.float32 if head in (K.HEAD_GAUSSIAN, K.HEAD_BERNOULLI) else torch.int64,
                              device=self.device)
            a.action_out = out.data_ptr()
            st = self._infer_state = dict(E=E, params=self.policy_params.data_ptr(), args=a, out=out)
        a = st["args"]
        K._req(t_obs.is_cuda and t_obs.dtype == torch.float32 and t_obs.numel() == E * a.actor.in_dim,
               "get_inference_actions: obs must hold [E, obs_dim] float32 values")
        t_obs = t_obs.contiguous()
        a.obs = t_obs.data_ptr()
        a.mode = K.INFER_DETERMINISTIC if deterministic else K.INFER_SAMPLE
        if not deterministic:
            per_row = {K.HEAD_MULTI_CATEGORICAL: a.n_action_slices, K.HEAD_BERNOULLI: a.actor.out_dim}.get(a.head_kind, 1)
            a.seed, a.offset = self.eval_rng().take(E * per_row)
        K.policy_infer(a)
        return st["out"]

    def get_inference_actions(self, obs, deterministic):
        """
        ppo_policy.py:796-889 -> the environment action of every row: the distribution's refined prediction when
        `deterministic`, else a sample.  numpy in -> numpy out, device tensor in -> device tensor out.  On K19 (see
        inference_unsupported_reason) and on K21 (an LSTM policy, see lstm_step_unsupported_reason; the actor's hidden
        state is stepped in place) the result is a reusable tensor that the next call overwrites.
        """
        if len(obs.shape) < 2:
            raise ValueError(f"get_inference_actions expects a batch of observations, got shape {obs.shape}")
        as_numpy = not torch.is_tensor(obs)
        t_obs = self._to_device(obs)
        if self.inference_unsupported_reason() == "":
            action = self._infer_step(t_obs, deterministic)
        elif self.using_lstm and self.lstm_step_unsupported_reason() == "":
            action = self._lstm_infer_step(t_obs, deterministic)
        else:
            dist = self.actor.distribution
            with torch.no_grad():
                pred = self.actor.forward_logits(t_obs)
                if deterministic:
                    action = dist.refine_prediction(pred)
                else:
                    rng, dist.rng = dist.rng, self.eval_rng()
                    try:
                        action = dist.sample_distribution(pred)[0]
                    finally:
                        dist.rng = rng
        return action.cpu().numpy() if as_numpy else action

    def get_critic_values(self, obs):
        """ppo_policy.py:1057-1071."""
        return self.critic(obs)

    def add_episode_info(self, agent_id, critic_observations, observations, next_observations,
                         raw_actions, actions, values, log_probs, rewards, where_done):
        """ppo_policy.py:545-651: one env step of E transitions for `agent_id` -> row t of the buffer."""
        col = self._agent_col[agent_id]
        E = self.env_batch_size
        self.buffer.write_step(self._t, slice(col * E, (col + 1) * E), critic_observations,
                               observations, next_observations, raw_actions, actions, values,
                               log_probs, rewards)
        self._agents_written += 1
        if self._agents_written == len(self.agent_ids):      # every agent of this policy has logged step t
            self._agents_written = 0
            self._t += 1

    def end_episodes(self, agent_id, env_idxs, episode_lengths, terminal, ending_values, ending_rewards):
        """
        ppo_policy.py:653-712.  Called after add_episode_info of the same step.
        ending_values / ending_rewards may have one entry per env_idx (what the
        terminal case passes, ppo.py:1817-1819) or one per env (what the
        bootstrapped case passes, ppo.py:1937-1938).  In the second form the
        reference indexes them by POSITION in env_idxs (ppo_policy.py:684-689),
        i.e. env i can receive env j's bootstrap (quirk Q1); here each env gets
        its own value.  The two coincide whenever env_idxs == arange(E).
        """
        if self.frozen:
            return
        col = self._agent_col[agent_id]
        E = self.env_batch_size
        idx = self._to_device(env_idxs, torch.int64).reshape(-1)
        if idx.numel() == 0:
            return
        ev = self._to_device(ending_values).reshape(-1)
        er = self._to_device(ending_rewards).reshape(-1)
        if ev.numel() == E and idx.numel() != E:
            ev = ev[idx]
        if er.numel() == E and idx.numel() != E:
            er = er[idx]
        t = self._t - 1 if self._agents_written == 0 else self._t
        self.buffer.mark_ends(t, idx + col * E, self._to_device(terminal, torch.bool).reshape(-1), ev, er)

    def finalize_dataset(self):
        """ppo_policy.py:714-719."""
        self.dataset.build()

    def clear_dataset(self):
        """ppo_policy.py:721-727 (the HBM buffer is kept for the next rollout)."""
        self.dataset = None

    def get_bs_clip_range(self, ep_rewards):
        """ppo_policy.py:1086-1112."""
        if not self.have_bootstrap_clip:
            return None
        if self.dynamic_bs_clip:
            # :1104-1106: (min, max) of the episode's own rewards.  The device buffer resolves it per episode
            # segment in RolloutBuffer.compute_advantages; this marker selects that path.
            return "dynamic"
        return (self.bootstrap_clip[0](), self.bootstrap_clip[1]())

    # ----------------------------------------------------------------- update
    def evaluate(self, batch_critic_obs, batch_obs, batch_actions):
        """ppo_policy.py:891-952 -> (values, log_probs [B,1], entropy [B])."""
        values = self.critic(batch_critic_obs).squeeze()
        pred = self.actor.forward_logits(batch_obs)
        log_probs, entropy = self.actor.distribution.get_log_probs_and_entropy(pred, batch_actions)
        return values, log_probs, entropy

    def update_weights(self, actor_loss, critic_loss):
        """ppo_policy.py:1012-1055."""
        if self.frozen:
            return
        scale = 1.0 / mpi_utils.get_num_procs()
        self.policy_grads.zero_()
        actor_loss.backward()
        critic_loss.backward()
        mpi_utils.allreduce_sum_(self.policy_grads)        # actor + critic in one message
        self.actor_optim.step(grad_scale=scale, max_norm=self.gradient_clip)
        self.critic_optim.step(grad_scale=scale, max_norm=self.gradient_clip)

    def optimizer_step(self, grad_scale):
        """clip + Adam for both networks (the tail of update_weights, on already averaged-by-sum gradients)."""
        self.actor_optim.step(grad_scale=grad_scale, max_norm=self.gradient_clip)
        self.critic_optim.step(grad_scale=grad_scale, max_norm=self.gradient_clip)

    def update_learning_rate(self):
        """ppo_policy.py:1073-1084."""
        if self.frozen:
            return
        self.actor_optim.set_lr(self.lr())
        self.critic_optim.set_lr(self.lr())
        if self.enable_icm:
            self.icm_optim.set_lr(self.icm_lr())

    # ------------------------------------------------------------- save / load
    def save(self, save_path, tag="latest"):
        """ppo_policy.py:1215-1247 (`<name>-policy/<tag>/{actor,critic}_<rank>.model`, `*_optim_<rank>`)."""
        policy_save_path = os.path.join(save_path, f"{self.name}-policy", str(tag))     # :1164-1165: any tag type
        os.makedirs(policy_save_path, exist_ok=True)
        self.actor.save(policy_save_path)
        self.critic.save(policy_save_path)
        if self.enable_icm:
            self.icm_model.save(policy_save_path)
        r = mpi_utils.get_rank()
        torch.save(self.actor_optim.state_dict(), os.path.join(policy_save_path, f"actor_optim_{r}"))
        torch.save(self.critic_optim.state_dict(), os.path.join(policy_save_path, f"critic_optim_{r}"))
        if self.enable_icm:
            torch.save(self.icm_optim.state_dict(), os.path.join(policy_save_path, f"icm_optim_{r}"))

    def load(self, load_path, tag="latest"):
        policy_load_path = os.path.join(load_path, f"{self.name}-policy", str(tag))
        self.actor.load(policy_load_path)
        self.critic.load(policy_load_path)
        if self.enable_icm:
            self.icm_model.load(policy_load_path)
        r = mpi_utils.get_rank()
        opts = [("actor", self.actor_optim), ("critic", self.critic_optim)]
        if self.enable_icm:
            opts.append(("icm", self.icm_optim))
        for net, opt in opts:
            f = os.path.join(policy_load_path, f"{net}_optim_{r}")
            if not os.path.exists(f):
                f = os.path.join(policy_load_path, f"{net}_optim_0")
            if net == "icm" and not os.path.exists(f):
                continue                                   # checkpoints written before the ICM optimiser was saved
            opt.load_state_dict(torch.load(f, map_location="cpu", weights_only=False))

    def direct_load(self, policy_load_path):
        """ppo_policy.py:1287-1300: networks only, from the directory itself (no `<name>-policy/<tag>` below it)."""
        self.actor.load(policy_load_path)
        self.critic.load(policy_load_path)
        if self.enable_icm:
            self.icm_model.load(policy_load_path)

    # ------------------------------------------------------------- hooks
    def apply_step_constraints(self, *args):
        """ppo_policy.py:1114-1135: identity; policies that must alter what the environment returns override it
        (args = obs, critic_obs, reward, terminated, truncated, info as PPO.apply_policy_step_constraints passes them)."""
        return args

    def apply_reset_constraints(self, *args):
        """ppo_policy.py:1137-1151: identity (args = obs, critic_obs)."""
        return args

    def get_agent_shared_intrinsic_rewards(self, *args):
        """ppo_policy.py:1009-1010: only agent-grouped policies can share an ICM."""
        raise NotImplementedError

    def __eq__(self, other):
        return isinstance(other, PPOPolicy) and self.name == other.name
