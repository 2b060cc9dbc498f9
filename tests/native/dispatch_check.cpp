// Host build of the launch plans (b747_rl_ctrl_amd/csrc/b747_dispatch.h: the header the entry points of libb747.so
// decide with), so that the CPU suite checks kernel choice and workgroup geometry without a GPU.  Compiled with plain
// g++ by tests/test_dispatch_plan.py, as tests/native/stepinfo_check.cpp is by its test.
#include "../../b747_rl_ctrl_amd/csrc/b747_dispatch.h"

using namespace b747;

extern "C" {

// out: kernel, x_f64, mix, sub, k1, envs_per_wg
void b747h_plan_env(const b747_env_batch *b, const b747_env_config *cfg, int32_t default_consts, int32_t spec,
                    int32_t n_env_steps, int32_t *out)
{
    const EnvPlan p = plan_env(*b, *cfg, default_consts != 0, spec, n_env_steps);
    out[0] = (int32_t)p.kernel; out[1] = p.x_f64; out[2] = p.mix; out[3] = p.sub; out[4] = p.k1; out[5] = p.envs_per_wg;
}

// out: kernel (0 k_model_step, 1 k_model_step_split, 2 k_model_steps_split), x_f64, envs_per_wg
void b747h_plan_model(const b747_model_batch *b, int32_t default_consts, int32_t spec, int32_t n_steps, int32_t *out)
{
    const ModelPlan p = plan_model(*b, default_consts != 0, spec, n_steps);
    out[0] = (int32_t)p.kernel; out[1] = p.x_f64; out[2] = p.envs_per_wg;
}

// returns ppo_rollout_covers; out: mix, sub, envs_per_wg of the rollout's plan
int32_t b747h_plan_ppo_rollout(const b747_env_batch *b, const b747_env_config *cfg, int32_t default_consts, int32_t *out)
{
    const PpoPlan p = plan_ppo_rollout(*b, *cfg);
    out[0] = p.mix; out[1] = p.sub; out[2] = p.envs_per_wg;
    return ppo_rollout_covers(*b, *cfg, default_consts != 0);
}

int32_t b747h_is_default(const b747_consts *c) { return is_default(*c); }

}  // extern "C"
