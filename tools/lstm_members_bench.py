"""
Rollout cost of an LSTM member in a multi-policy run on one GPU (profiles/lstm_members.txt):

  mpe_simple_adversary's dims -- an adversary (O 8) on an LSTM PPOPolicy (LSTM width 32, ff 16, sequence_length 5), two
  agents (O 10) on a MATPolicy team, Discrete(5), E = 4096, T = 128, max_ts_per_ep = 25 (the scenario's episode
  length: the LSTM critic's extra step runs after every env step), update_mode="fused", PPO.lstm_members = True --

  blocks          K21 on the env's row blocks (ppoaf_lstm_policy_step_blocks), K16 on its block form, K23
  lstm gathered   the same, but the LSTM member alone on gathered rows (its table is refused through
                  lstm_step_blocks_unsupported_reason, the fall-back a refused table takes)
  all gathered    PPO.step_row_blocks = False: both members gather their rows and index_put their actions

alternated in one process.  Per leg: median rollout milliseconds of --repeats rollouts (after one warm-up) with the spread
(min .. max), and what the package issues per env step (tools/mixed_policies_bench.py:per_step_counts).

    python tools/lstm_members_bench.py [--envs 4096] [--ts 128] [--repeats 5] [--label this]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mixed_policies_bench import DEV, box, per_step_counts, report, timed               # noqa: E402
from ppo_and_friends_amd.environments.synthetic import SyntheticMixedAgentsEnv          # noqa: E402
from ppo_and_friends_amd.networks.lstm import LSTMNetwork                               # noqa: E402
from ppo_and_friends_amd.policies.mat_policy import MATPolicy                           # noqa: E402
from ppo_and_friends_amd.ppo import PPO                                                 # noqa: E402
from ppo_and_friends_amd.spaces import Discrete                                         # noqa: E402


def make(E, T):
    specs = [("adversary_0", 8, Discrete(5)), ("agent_0", 10, Discrete(5)), ("agent_1", 10, Discrete(5))]
    env_gen = lambda: SyntheticMixedAgentsEnv(E, specs, T, DEV, reward="uniform", seed=33)
    kw = dict(sequence_length=5, lstm_hidden_size=32, ff_hidden_size=16)
    lstm = dict(ac_network=LSTMNetwork, actor_kw_args=dict(kw), critic_kw_args=dict(kw))
    settings = {"adversary": (None, box(8), box(8), Discrete(5), lstm), "team": (MATPolicy, box(10), box(10), Discrete(5), {})}
    ppo = PPO(env_gen, settings, policy_mapping_fn=lambda a: "adversary" if a.startswith("adversary") else "team",
              device=DEV, random_seed=8, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
              batch_size=256, max_ts_per_ep=25, update_mode="fused", save_state=False)
    ppo.lstm_members = True
    return ppo


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--ts", type=int, default=128)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--label", default="this")
    a = p.parse_args()
    E, T = a.envs, a.ts
    ppo = make(E, T)
    pol = ppo.policies["adversary"]
    own_reason = pol.lstm_step_blocks_unsupported_reason

    def leg(blocks, lstm_blocks):
        def set_up():
            ppo.step_row_blocks = blocks
            pol.lstm_step_blocks_unsupported_reason = own_reason if lstm_blocks else \
                (lambda *tables: "bench leg: the LSTM member on gathered rows")
        return set_up

    legs = {"blocks": leg(True, True), "lstm gathered": leg(True, False), "all gathered": leg(False, False)}

    def rollout_ms(set_up):
        def run():
            set_up()
            ppo.rollout()
            return ppo.status_dict["global status"]["rollout time"] * 1e3
        return run

    print(f"# {a.label}: E={E} T={T}, {torch.cuda.get_device_name(0)}; LSTM adversary + MAT team; rollout time as PPO.rollout "
          "reports it (synchronised)")
    ms = timed({k: rollout_ms(v) for k, v in legs.items()}, a.repeats)
    for name, set_up in legs.items():
        set_up()
        report(a.label, name, ms[name], per_step_counts(ppo, T))
    assert getattr(pol, "_lstm_blocks_table", None) is not None, "the block form never ran"


if __name__ == "__main__":
    main()
