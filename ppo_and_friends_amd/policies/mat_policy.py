"""
MATPolicy -- the Multi-Agent-Transformer policy surface (policies/mat_policy.py:24-1086 of the
reference) on the device rollout buffer.

Same hooks as the reference: agent_grouping = True, one actor_critic network and ONE optimiser
(summed actor + critic loss, one clip over all parameters: mat_policy.py:677-699), the critic
encodes the whole agent sequence once and the decoder samples the agents autoregressively during
rollouts (:441-519), evaluation is teacher-forced with the shifted one-hot action block (:378-439),
use_huber_loss defaults to True (:27-29).

Layout: a dataset row is one env step of one env with its A agents side by side
([A, .] items of PPOSharedEpisodeDataset); tensors are [rows, A, .] on the device.  The attention
core is the f32-MFMA kernel K9; linears / LayerNorm / GELU are torch-ROCm.  Rollout steps (K16), mini-batch updates
(K15) and evaluation steps (K20) of the covered shapes are one launch each.
"""
import numpy as np
import torch
import torch.nn.functional as t_func

from ..networks.multi_agent_transformer import MATActorCritic
from ..spaces import get_agent_shared_space, get_space_shape
from ..utils import mpi_utils
from ..utils.episode_info import PPODataset, RolloutBuffer
from .ppo_policy import FlatAdam, PPOPolicy


class MATPolicy(PPOPolicy):

    def __init__(self, ac_network=MATActorCritic, mat_kw_args={}, use_huber_loss=True, **kw_args):
        super().__init__(ac_network=ac_network, mat_kw_args=mat_kw_args, use_huber_loss=use_huber_loss, **kw_args)
        self.agent_grouping = True
        self.expanded_actor_space = False
        if get_space_shape(self.actor_obs_space) != get_space_shape(self.critic_obs_space):
            # mat_policy.py:75-79: the actor then sees the critic's (wider) observation
            self.expanded_actor_space = True
            self.have_step_constraints = True
            self.have_reset_constraints = True
            self.actor_obs_space = self.critic_obs_space

    # ------------------------------------------------------------------ setup
    def finalize(self, status_dict, device):
        """mat_policy.py:191-245."""
        if len(self.agent_ids) == 0:
            self.register_agent("agent0")
        self._env_agent_index = {a: i for i, a in enumerate(self.agent_ids)}    # env's agent order
        self.agent_idxs = np.arange(len(self.agent_ids))
        self.num_agents = self.agent_idxs.size
        self.device = torch.device(device)
        self._initialize_networks(**self.network_args)
        for c in (self.lr, self.icm_lr, self.entropy_weight, self.intr_reward_weight):
            c.finalize(status_dict)
        if self.have_bootstrap_clip:
            self.bootstrap_clip[0].finalize(status_dict)
            self.bootstrap_clip[1].finalize(status_dict)
        self.actor_critic_optim = FlatAdam(self.actor_critic, self.lr(), eps=1e-5)
        self.icm_optim = FlatAdam(self.icm_model, self.icm_lr(), eps=1e-5) if self.enable_icm else None   # mat_policy.py:224-227
        self.shuffle_agent_ids()

    def _initialize_networks(self, ac_network, enable_icm, icm_network, mat_kw_args, icm_kw_args, **kw_args):
        """mat_policy.py:88-176."""
        if not issubclass(ac_network, MATActorCritic):
            raise TypeError(f"ac_network for MATPolicy must be a subtype of MATActorCritic, got {ac_network}")
        self.actor_critic = ac_network(name="actor_critic", obs_space=self.critic_obs_space,
                                       action_space=self.action_space, num_agents=len(self.agent_ids),
                                       test_mode=self.test_mode,
                                       seed=self.random_seed + 7919 * mpi_utils.get_rank(), **mat_kw_args)
        self.actor_critic.to(self.device)
        mpi_utils.broadcast_model_parameters(self.actor_critic)
        self.actor = self.actor_critic.actor
        self.critic = self.actor_critic.critic
        self.policy_params = self.actor_critic.flat_params
        self.policy_grads = self.actor_critic.flat_grads
        if enable_icm:
            # mat_policy.py:132-176.  Two forms: one ICM over each agent's own (observation, action) -- rows are
            # then (env, agent) pairs -- or, with agent_shared_icm, one ICM over the concatenation of the
            # group's observations / actions in the ORIGINAL agent order (icm_agent_ids), one reward per env.
            from ..networks.icm import ICM
            self.icm_agent_ids = None
            icm_obs_space, icm_action_space = self.actor_obs_space, self.action_space
            if self.agent_shared_icm:
                if self.expanded_actor_space:
                    raise ValueError("agent_shared_icm can only be enabled with the multi-agent transformer "
                                     "if critic view is set to local (mat_policy.py:146-152)")
                n = len(self.agent_ids)
                icm_obs_space = get_agent_shared_space(self.actor_obs_space, n)
                icm_action_space = get_agent_shared_space(self.action_space, n)
                self.icm_agent_ids = np.array(self.agent_ids).copy()
            icm_cls = ICM if icm_network is None else icm_network
            self.icm_model = icm_cls(name="icm", obs_space=icm_obs_space, action_space=icm_action_space,
                                     test_mode=self.test_mode, **icm_kw_args)
            self.icm_model.to(self.device)
            mpi_utils.broadcast_model_parameters(self.icm_model)

    def agent_slot_order(self):
        """Index of the env's agent that sits in each slot of the grouped rows (after the MAT shuffles)."""
        return np.array([self._env_agent_index[a] for a in self.agent_ids], dtype=np.int64)

    def to(self, device):
        self.device = torch.device(device)
        self.actor_critic.to(self.device)

    def eval(self):
        self.actor_critic.eval()

    def train(self):
        self.actor_critic.train()

    # ---------------------------------------------------------------- rollout
    def initialize_dataset(self):
        """mat_policy.py:179-189 (PPOSharedEpisodeDataset: rows of [A, .])."""
        self.dataset = PPODataset(device=self.device, action_dtype=self.action_dtype, sequence_length=1)
        self.dataset.shared = True
        # quirk Q14 (replicated; pinned by fixture g12_c5_mat): the reference creates the dataset BEFORE the rollout
        # reshuffles the agents (ppo.py:1546-1547 vs 1643-1644) and PPOSharedEpisodeDataset keeps the agent_ids array it
        # was handed (episode_info.py:1012), so the dataset's agent axis stays in the order the policy had at this point
        self._dataset_slot_order = self.agent_slot_order()

    def finalize_dataset(self):
        """ppo_policy.py:714-719, with the dataset's agent axis put into its creation-time order (quirk Q14)."""
        rollout_order = self.agent_slot_order()
        want = getattr(self, "_dataset_slot_order", rollout_order)
        if not np.array_equal(want, rollout_order):
            k = torch.as_tensor(np.argsort(rollout_order)[want], device=self.device)      # dataset slot j <- rollout slot k[j]
            b = self.buffer
            for name in ("observations", "critic_observations", "next_observations", "actions", "raw_actions", "values",
                         "log_probs", "rewards", "boot_value", "boot_reward"):
                x = getattr(b, name)
                if x is not None:
                    x.copy_(x.index_select(2, k))
            if getattr(b, "boot_stats", None) is not None:
                b.boot_stats = b.boot_stats.index_select(2, k)
        self.dataset.build()

    def initialize_episodes(self, env_batch_size, status_dict, ts_per_rollout=None):
        if ts_per_rollout is None:
            raise ValueError("initialize_episodes needs ts_per_rollout (total steps over all envs)")
        T = int(ts_per_rollout) // int(env_batch_size)
        self.env_batch_size = int(env_batch_size)
        A = len(self.agent_ids)
        if A < 2:
            raise NotImplementedError("MATPolicy groups the agents of an env into one sequence: it needs at least two "
                                      "agents (a single agent is an ordinary PPOPolicy)")
        obs_dim = int(np.prod(get_space_shape(self.actor_obs_space)))
        cobs_dim = int(np.prod(get_space_shape(self.critic_obs_space)))
        if self.buffer is None or (self.buffer.T, self.buffer.C) != (T, self.env_batch_size):
            self.buffer = RolloutBuffer(T, self.env_batch_size, obs_dim, cobs_dim, self.action_dim,
                                        self.action_dtype, self.device, keep_next_observations=self.enable_icm,
                                        agents_per_row=A)
        else:
            self.buffer.end_kind.zero_()
            self.buffer.fixed_length = True
            self.buffer.steps_written = 0
        self._t = 0
        self.dataset.attach(self.buffer, self.gamma, self.lambd, self.get_bs_clip_range(None), self.use_gae)

    def fused_step_unsupported_reason(self):
        """'' when the K16 rollout-step kernel covers this policy (same coverage as the fused update K15)."""
        from ..fused_update import _describe_mat
        return _describe_mat(self)[1]

    def rollout_step(self, t, critic_obs, actor_obs, value_normalizer=None, forced_raw_action=None, blocks=None):
        """
        blocks (optional, then critic_obs / actor_obs are None): (critic_obs_blocks, actor_obs_blocks or None,
        env_action_blocks), one device tensor per agent of the policy in env order -- the [E, .] rows of the env's tensors
        where they lie and its int64 action tensors [E] / [E, 1], which the launch fills beside the grouped buffer row
        (ppoaf_mat_policy_step_blocks reads them in the policy's slot order); `step_blocks_unsupported_reason` says when not.
        forced_raw_action (optional int64 device tensor [E, A] / [E, A, 1]): log these actions instead of sampling
        (replay of a recorded rollout).
        One env step of get_rollout_actions (encoder + A autoregressive decoder passes + sampling) and
        get_critic_values (+ denormalisation) as ONE launch (K16) that stores straight into row t of the
        rollout buffer.  critic_obs / actor_obs: grouped device tensors [E, A, .].  Returns the action row
        (a view of the buffer, [E, A, 1]) for env.step; rewards are added by `finish_step`.
        """
        from .. import _lib
        from .. import kernels as K
        from ..fused_update import _describe_mat
        import ctypes as C
        buf = self.buffer
        E, A = buf.C, buf.A
        a = getattr(self, "_step_args", None)
        if a is None:
            topo, why = _describe_mat(self)
            if topo is None:
                raise _lib.PpoafError(f"mat rollout_step: {why}")
            a = _lib.MatStepArgs()
            a.obs_dim, a.num_agents, a.num_actions, a.embedding = topo["obs_dim"], topo["num_agents"], topo["num_actions"], 64
            for i, o in enumerate(topo["offsets"]):
                a.offsets[i] = o
            a.params = self.actor_critic.flat_params.data_ptr()
            a.E = E
            a.actor_obs_dim = int(buf.observations.shape[-1])
            self._step_args = a
        if blocks is not None:
            why = self.step_blocks_unsupported_reason(*blocks)
            if why:
                raise _lib.PpoafError(f"mat rollout_step: {why}")
            tb = getattr(self, "_step_blocks", None)
            if tb is None:
                tb = self._step_blocks = _lib.MatStepBlocks()
            tb.n_blocks = A
            for s_, b in enumerate(self.agent_slot_order()):
                tb.slot_agent[s_] = int(b)
            for b in range(A):
                tb.critic_obs[b], tb.env_action[b] = blocks[0][b].data_ptr(), blocks[2][b].data_ptr()
                tb.actor_obs[b] = None if blocks[1] is None else blocks[1][b].data_ptr()
            a.critic_obs = a.actor_obs = None
        else:
            if critic_obs.shape != (E, A, a.obs_dim) or not critic_obs.is_cuda:
                raise _lib.PpoafError(f"mat rollout_step: critic_obs must be a device tensor [{E}, {A}, {a.obs_dim}]")
            critic_obs = critic_obs.contiguous()
            actor_obs = actor_obs.contiguous()
            a.critic_obs, a.actor_obs = critic_obs.data_ptr(), actor_obs.data_ptr()
        a.seed, a.offset = self.actor.distribution.rng.take(E * A)
        a.forced_action = None
        if forced_raw_action is not None:
            if not (forced_raw_action.is_cuda and forced_raw_action.dtype == torch.int64 and forced_raw_action.is_contiguous()
                    and forced_raw_action.numel() == E * A):
                raise _lib.PpoafError(f"mat rollout_step: forced_raw_action must be a contiguous int64 device tensor [{E}, {A}]")
            a.forced_action = forced_raw_action.data_ptr()
        a.normalize_values = int(value_normalizer is not None)
        if value_normalizer is not None:
            a.vn_mean = value_normalizer.running_stats.mean_t.data_ptr()
            a.vn_var = value_normalizer.running_stats.var_t.data_ptr()
        a.action_out, a.raw_action_out = buf.actions[t].data_ptr(), buf.raw_actions[t].data_ptr()
        a.logp_out, a.value_out = buf.log_probs[t].data_ptr(), buf.values[t].data_ptr()
        a.critic_obs_copy_out, a.obs_copy_out = buf.critic_observations[t].data_ptr(), buf.observations[t].data_ptr()
        if blocks is not None:
            _lib.check(_lib.load().ppoaf_mat_policy_step_blocks(C.byref(a), C.byref(tb), K.stream()), "mat_policy_step_blocks")
        else:
            _lib.check(_lib.load().ppoaf_mat_policy_step(C.byref(a), K.stream()), "mat_policy_step")
        return buf.actions[t]

    def step_blocks_unsupported_reason(self, critic_obs_blocks, actor_obs_blocks, env_action_blocks):
        """'' when ppoaf_mat_policy_step_blocks takes these per-agent blocks (the library checks the same before it launches)."""
        from .. import _lib
        buf = self.buffer
        E, A = buf.C, buf.A
        if not 1 <= A <= _lib.ROW_BLOCKS_MAX:
            return f"{A} agents, a row-block table holds {_lib.ROW_BLOCKS_MAX}"
        sets = [("critic observation", critic_obs_blocks, torch.float32, buf.critic_observations.shape[-1]),
                ("env action", env_action_blocks, torch.int64, 1)]
        if actor_obs_blocks is not None:
            sets.append(("observation", actor_obs_blocks, torch.float32, buf.observations.shape[-1]))
        for what, blks, dt, width in sets:
            if len(blks) != A:
                return f"{len(blks)} {what} blocks for {A} agents"
            for b, x in enumerate(blks):
                if not (torch.is_tensor(x) and x.is_cuda and x.dtype == dt and x.is_contiguous() and x.numel() == E * width):
                    return f"{what} block {b} is not a contiguous {dt} device tensor of {E} x {width}"
                if x.data_ptr() % 16:
                    return f"{what} block {b} does not start on a 16-byte boundary"
        return ""

    def finish_step(self, t, rewards, next_obs=None):
        buf = self.buffer
        if rewards is not None:           # None: K23 has written the row already
            buf.rewards[t].copy_(rewards.reshape(buf.rewards[t].shape))
        if buf.next_observations is not None and next_obs is not None:
            buf.next_observations[t].copy_(next_obs.reshape(buf.next_observations[t].shape))
        buf.steps_written = max(buf.steps_written, t + 1)
        self._t = t + 1

    def _get_tokened_action_block(self, batch_size):
        """mat_policy.py:308-344."""
        A = len(self.agent_ids)
        if self.action_dtype == "continuous":
            return torch.zeros((batch_size, A, self.action_pred_size), device=self.device)
        blk = torch.zeros((batch_size, A, self.action_pred_size + 1), device=self.device)
        blk[:, 0, 0] = 1
        return blk

    def _get_autoregressive_actions(self, encoded_obs, forced_raw_action=None):
        """mat_policy.py:441-519: A decoder passes, agent i conditioned on the actions of agents < i.
        forced_raw_action [B, A, .]: recorded raw actions to log instead of sampling (replay)."""
        B, A = encoded_obs.shape[0], len(self.agent_ids)
        block = self._get_tokened_action_block(B)
        off = 1 if self.action_dtype == "discrete" else 0
        adt = torch.int64 if self.action_dtype == "discrete" else torch.float32
        out_a = torch.zeros((B, A, self.action_dim), dtype=adt, device=self.device)
        out_raw = torch.zeros_like(out_a)
        out_lp = torch.zeros((B, A, 1), dtype=torch.float32, device=self.device)
        with torch.no_grad():
            for i in range(A):
                pred = self.actor(block, encoded_obs)[:, i, :].contiguous()
                if forced_raw_action is None:
                    action, raw_action, log_prob = self.actor.distribution.sample_distribution(pred)
                else:
                    raw_action = forced_raw_action.reshape(B, A, -1)[:, i, :].contiguous()
                    log_prob, _ = self.actor.distribution.get_log_probs_and_entropy(pred, raw_action)
                    action = raw_action if self.action_dtype == "discrete" else self.actor.distribution.refine_prediction(raw_action)
                out_a[:, i, :] = action.reshape(B, self.action_dim)
                out_raw[:, i, :] = raw_action.reshape(B, self.action_dim)
                out_lp[:, i, :] = log_prob.reshape(B, 1)
                if i + 1 < A:
                    if self.action_dtype == "discrete":
                        block[:, i + 1, off:] = t_func.one_hot(action.reshape(B), num_classes=self.action_pred_size).float()
                    else:
                        block[:, i + 1, off:] = action.reshape(B, -1)
        return out_a, out_raw, out_lp

    def get_rollout_actions(self, obs, forced_raw_action=None):
        """
        mat_policy.py:587-626.  Device tensors arrive grouped, [E, A, O], and grouped tensors are
        returned ([E, A, .]); numpy arrives in the reference's [A, E, O] and is swapped like there.
        """
        as_numpy = not torch.is_tensor(obs)
        t_obs = self._to_device(np.swapaxes(obs, 0, 1) if as_numpy else obs)
        with torch.no_grad():
            encoded_obs, _ = self.critic(t_obs)
        actions, raw_actions, log_probs = self._get_autoregressive_actions(encoded_obs, forced_raw_action)
        if as_numpy:
            return (torch.swapaxes(raw_actions, 0, 1).cpu().numpy(), torch.swapaxes(actions, 0, 1).cpu().numpy(),
                    torch.swapaxes(log_probs, 0, 1).detach())
        return raw_actions, actions, log_probs

    def _get_autoregressive_actions_without_exploration(self, encoded_obs):
        """mat_policy.py:521-585: the greedy decode -- agent i takes the refined prediction of its distribution,
        conditioned on the refined actions of agents < i.  -> actions [B, A, action_dim]."""
        B, A = encoded_obs.shape[0], len(self.agent_ids)
        block = self._get_tokened_action_block(B)
        off = 1 if self.action_dtype == "discrete" else 0
        adt = torch.int64 if self.action_dtype == "discrete" else torch.float32
        out_a = torch.zeros((B, A, self.action_dim), dtype=adt, device=self.device)
        with torch.no_grad():
            for i in range(A):
                pred = self.actor(block, encoded_obs)[:, i, :].contiguous()
                action = self.actor.distribution.refine_prediction(pred)
                out_a[:, i, :] = action.reshape(B, self.action_dim)
                if i + 1 < A:
                    if self.action_dtype == "discrete":
                        block[:, i + 1, off:] = t_func.one_hot(action.reshape(B), num_classes=self.action_pred_size).float()
                    else:
                        block[:, i + 1, off:] = action.reshape(B, -1)
        return out_a

    def inference_unsupported_reason(self):
        """'' when get_inference_actions runs on K20 (ppoaf_mat_policy_infer: the coverage of K16 and K15, on a device
        policy that PPO has not put on the torch path), else why the network modules decode."""
        if self.device.type != "cuda":
            return f"the policy lives on {self.device}: K20 needs a HIP device"
        if getattr(self, "update_mode", "auto") == "torch":
            return "update_mode='torch' keeps the policy on the torch-ROCm path"
        # (asked once per evaluation step: the answer is kept for as long as the parameter bucket stays)
        key = self.policy_params.data_ptr()
        if getattr(self, "_infer_reason", (None, ""))[0] != key:
            from ..fused_update import MAT_INFER_MAX_OBS
            why, O = self.fused_step_unsupported_reason(), self.critic.in_size
            if not why and O > MAT_INFER_MAX_OBS:
                why = f"observations {O} wide: the K20 evaluation step takes up to {MAT_INFER_MAX_OBS} (K15 and K16 take these)"
            self._infer_reason = (key, why)
        return self._infer_reason[1]

    def _infer_step(self, t_obs, deterministic, agent_major=False):
        """
        K20: one launch, encoder + A decoder passes -> env actions, into a reusable output tensor.  t_obs holds E * A
        observation rows, grouped ([E, A, O], slot order; -> [E, A, 1]) or, with agent_major, as the env hands them
        ([A * E, O], env agent order; -> [A * E, 1]): the slot order then travels in the arguments.
        """
        from .. import _lib
        from .. import kernels as K
        from ..fused_update import _describe_mat
        A = len(self.agent_ids)
        st = getattr(self, "_infer_state", None)
        if st is None or st["params"] != self.policy_params.data_ptr():
            topo, why = _describe_mat(self)
            if topo is None:
                raise _lib.PpoafError(f"mat inference step: {why}")
            a = _lib.MatInferArgs()
            a.obs_dim, a.num_agents, a.num_actions, a.embedding = topo["obs_dim"], topo["num_agents"], topo["num_actions"], 64
            for i, o in enumerate(topo["offsets"]):
                a.offsets[i] = o
            a.params = self.policy_params.data_ptr()
            st = self._infer_state = dict(params=a.params, args=a, out={}, order=None)
        a = st["args"]
        K._req(t_obs.is_cuda and t_obs.dtype == torch.float32 and t_obs.numel() % (A * a.obs_dim) == 0,
               f"get_inference_actions: obs must hold [E, {A}, {a.obs_dim}] float32 values on the device")
        E = t_obs.numel() // (A * a.obs_dim)
        out = st["out"].get((E, agent_major))
        if out is None:
            out = st["out"][(E, agent_major)] = torch.zeros((A * E, 1) if agent_major else (E, A, 1), dtype=torch.int64,
                                                            device=self.device)
        order = tuple(self.agent_ids) if agent_major else None
        if st["order"] != (agent_major, order):
            for i, k in enumerate(self.agent_slot_order() if agent_major else range(A)):
                a.slot_agent[i] = int(k)
            st["order"] = (agent_major, order)
        a.E = E
        a.obs_env_stride, a.obs_agent_stride = (1, E) if agent_major else (A, 1)
        a.act_env_stride, a.act_agent_stride = a.obs_env_stride, a.obs_agent_stride
        t_obs = t_obs.contiguous()
        a.obs, a.action_out = t_obs.data_ptr(), out.data_ptr()
        a.mode = K.INFER_DETERMINISTIC if deterministic else K.INFER_SAMPLE
        if not deterministic:
            a.seed, a.offset = self.eval_rng().take(E * A)
        K.mat_policy_infer(a)
        return out

    def get_inference_actions(self, obs, deterministic):
        """
        mat_policy.py:701-790: encode once with the critic, then decode the agents one after the other -- sampled
        (from the evaluation's own Philox stream) or greedy.  Device tensors arrive grouped, [E, A, O], and [E, A, .]
        is returned; numpy arrives in the reference's [A, E, O] and is swapped like there.  On K20 (see
        inference_unsupported_reason) all of it is one launch and the result is a reusable tensor that the next call
        overwrites; else the network modules decode.
        """
        if len(obs.shape) < 3:
            raise ValueError(f"get_inference_actions expects a batch of grouped observations, got shape {obs.shape}")
        as_numpy = not torch.is_tensor(obs)
        t_obs = self._to_device(np.swapaxes(obs, 0, 1) if as_numpy else obs)
        if self.inference_unsupported_reason() == "":
            actions = self._infer_step(t_obs, deterministic)
            return torch.swapaxes(actions, 0, 1).cpu().numpy() if as_numpy else actions
        with torch.no_grad():
            encoded_obs, _ = self.critic(t_obs)
        if deterministic:
            actions = self._get_autoregressive_actions_without_exploration(encoded_obs)
        else:
            dist = self.actor.distribution
            rng, dist.rng = dist.rng, self.eval_rng()
            try:
                actions = self._get_autoregressive_actions(encoded_obs)[0]
            finally:
                dist.rng = rng
        return torch.swapaxes(actions, 0, 1).cpu().numpy() if as_numpy else actions

    def get_inference_actions_agent_major(self, obs, deterministic):
        """get_inference_actions on the env's own layout, K20 only: obs [A * E, O] (rows of env agent a at a * E ..) ->
        the env's action tensor [A * E, 1]; no regrouping on the host, the slot order is an argument of the launch."""
        return self._infer_step(obs, deterministic, agent_major=True)

    def get_critic_values(self, obs):
        """mat_policy.py:660-675."""
        _, values = self.critic(obs)
        return values

    # ----------------------------------------------------------------- update
    def evaluate(self, batch_critic_obs, batch_obs, batch_actions):
        """mat_policy.py:378-439,628-658 -> values [B,A,1], log_probs [B,A,1], entropy [B,A,1]."""
        B, A = batch_critic_obs.shape[0], len(self.agent_ids)
        block = self._get_tokened_action_block(B)
        if self.action_dtype == "discrete":
            acts = batch_actions.reshape(B, A)
            block[:, 1:, 1:] = t_func.one_hot(acts, num_classes=self.action_pred_size)[:, :-1, :].float()
        else:
            block[:, 1:, :] = batch_actions[:, :-1, :]
        values, pred = self.actor_critic(batch_critic_obs, block)
        pred = pred.reshape(-1, self.action_pred_size)
        flat_actions = batch_actions.reshape(-1, self.action_dim)
        log_probs, entropy = self.actor.distribution.get_log_probs_and_entropy(pred, flat_actions)
        return values, log_probs.reshape(B, A, -1), entropy.reshape(B, A, -1)

    def optimizer_step(self, grad_scale):
        self.actor_critic_optim.step(grad_scale=grad_scale, max_norm=self.gradient_clip)

    def update_weights(self, actor_loss, critic_loss):
        """mat_policy.py:677-699."""
        if self.frozen:
            return
        self.policy_grads.zero_()
        (actor_loss + critic_loss).backward()
        mpi_utils.allreduce_sum_(self.policy_grads)
        self.optimizer_step(1.0 / mpi_utils.get_num_procs())

    def update_learning_rate(self):
        if not self.frozen:
            self.actor_critic_optim.set_lr(self.lr())
            if self.enable_icm:                          # mat_policy.py:895-896
                self.icm_optim.set_lr(self.icm_lr())

    def save(self, save_path, tag="latest"):
        import os
        path = os.path.join(save_path, f"{self.name}-policy", str(tag))
        os.makedirs(path, exist_ok=True)
        self.actor_critic.save(path)                     # actor_critic_<rank>.model, as the reference
        torch.save(self.actor_critic_optim.state_dict(),
                   os.path.join(path, f"actor_critic_optim_{mpi_utils.get_rank()}"))
        if self.enable_icm:                              # mat_policy.py:1105-1111
            self.icm_model.save(path)
            torch.save(self.icm_optim.state_dict(), os.path.join(path, f"icm_optim_{mpi_utils.get_rank()}"))

    def load(self, load_path, tag="latest"):
        import os
        path = os.path.join(load_path, f"{self.name}-policy", str(tag))
        self.actor_critic.load(path)
        f = os.path.join(path, f"actor_critic_optim_{mpi_utils.get_rank()}")
        if not os.path.exists(f):
            f = os.path.join(path, "actor_critic_optim_0")
        self.actor_critic_optim.load_state_dict(torch.load(f, map_location="cpu", weights_only=False))
        if self.enable_icm:
            self.icm_model.load(path)
            f = os.path.join(path, f"icm_optim_{mpi_utils.get_rank()}")
            if not os.path.exists(f):
                f = os.path.join(path, "icm_optim_0")
            if os.path.exists(f):
                self.icm_optim.load_state_dict(torch.load(f, map_location="cpu", weights_only=False))

    def direct_load(self, policy_load_path):
        """mat_policy.py (direct_load): the networks only, from the directory itself."""
        self.actor_critic.load(policy_load_path)
        if self.enable_icm:
            self.icm_model.load(policy_load_path)

    def get_agent_shared_intrinsic_rewards(self, prev_obs, obs, actions):
        """
        mat_policy.py:1012-1090.  The reference takes dicts keyed by agent id and stacks them in
        icm_agent_ids order; here the environment's agent-major batches [A*E, .] (rows of agent a at
        a*E..(a+1)*E, the env's = the original agent order) are regrouped to [E, A*.]: one ICM row and one
        reward per env, already weighted.  Returns float32 [E].
        """
        A = len(self.agent_ids)
        obs_1 = self._to_device(prev_obs)
        if obs_1.dim() < 2:
            raise ValueError(f"get_agent_shared_intrinsic_rewards expects a batch of observations, got {obs_1.shape}")
        E = obs_1.shape[0] // A
        join = lambda x: x.reshape(A, E, -1).transpose(0, 1).reshape(E, -1)
        obs_1, obs_2 = join(obs_1), join(self._to_device(obs))
        adt = torch.int64 if self.action_dtype in ("discrete", "multi-discrete") else torch.float32
        act = join(self._to_device(actions, adt))
        if self.fused_shared_icm and obs_1.is_cuda and getattr(self, "fused_icm_reward", True):
            # K14 on the joined rows [E, A O] / int64 [E, A] (opt-in; counted in PPOPolicy.fused_icm_reward_calls)
            fused = self._fused_intrinsic_reward(obs_1, obs_2, act)
            if fused is not None:
                return fused
        with torch.no_grad():
            intr, _, _ = self.icm_model(obs_1, obs_2, act)
        return intr.reshape(-1) * float(self.intr_reward_weight())

    def apply_step_constraints(self, obs, critic_obs, reward, terminated, truncated, info):
        """
        mat_policy.py:808-853: with a non-local critic view the actor must see the critic's observation
        (`obs[agent] = critic_obs[agent]`).  This build makes that substitution where the observation is
        consumed -- the rollout hands the critic's observation to K16 / get_rollout_actions for the actor
        when `expanded_actor_space` is set (ppo.py rollout) -- so the env tuple passes through unchanged.
        """
        return obs, critic_obs, reward, terminated, truncated, info

    def apply_reset_constraints(self, obs, critic_obs):
        """mat_policy.py:855-878: see apply_step_constraints."""
        return obs, critic_obs
