// K21's device views of checked step arguments, shared by the kernels of lstm_policy_step.hip (hidden 32, 64, 128; tiles
// of 16 rows) and of lstm_wide_step.hip (hidden 256; tiles of 32 rows).  The entry points, their layout asserts and
// step_dev_of, which fills the view, stay in lstm_policy_step.hip.
#pragma once
#include "lstm_device.hpp"

namespace ppoaf {

struct LstmStepDev {
    LstmArgs net[2];                               // actor, critic
    long E;
    int n_wg, mode, head_kind, infer_mode;         // n_wg: row tiles of the launch's kernel (16 or 32 rows each)
    float min_std;
    const float* log_std;
    const float* act_lo; const float* act_hi;
    const void* forced_raw_action;
    unsigned long long seed, offset;
    int normalize_values; const float* vn_mean; const float* vn_var;
    void* raw_action_out; void* action_out; float* logp_out;
    float* value_out;                              // values[t] (STEP) or boot_value[t] (CRITIC_NEXT)
    float* obs_out; float* critic_obs_out;
    const unsigned char* terminated;
    float* stored[4];                              // the step's hidden rows, for the zeroing
};

// The block form (ppoaf_lstm_policy_step_blocks): row r of the launch is row r % rows_per_block of block
// r / rows_per_block of `obs` / `critic_obs`, its env action (STEP) also goes to that row of `env_action`, and
// `terminated` (CRITIC_NEXT) holds one byte per row of a block.  The pointers travel in the kernel arguments.
struct LstmStepBlocks {
    const float* obs[PPOAF_ROW_BLOCKS_MAX];
    const float* critic_obs[PPOAF_ROW_BLOCKS_MAX];
    void* env_action[PPOAF_ROW_BLOCKS_MAX];
    unsigned rows_per_block;
    int action_elems;                              // float32 elements of a Gaussian row's env action; int64: 1
};

// host: the launchers of lstm_wide_step.hip, called by K21's entry points at hidden == 256 (u.n_wg counts 32-row tiles)
int lstm_wide_step(const LstmStepDev& u, hipStream_t stream);
int lstm_wide_step_blocks(const LstmStepDev& u, const LstmStepBlocks& tb, hipStream_t stream);

}  // namespace ppoaf
