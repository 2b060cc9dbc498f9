// Host wrapper around the streaming step-response accumulator (b747_rl_ctrl_amd/csrc/b747_stepinfo.h) for
// tests/test_stepinfo_stream.py: feeds a series one sample at a time, as k_eval_episodes does per DLL step.
#include "../../b747_rl_ctrl_amd/csrc/b747_stepinfo.h"

extern "C" void stepinfo_stream(const double *ys, const double *ts, int n, double y_base, double error_band, double *out4)
{
    b747::StepInfoAcc acc;
    acc.init(y_base, error_band);
    for (int i = 0; i < n; ++i) acc.push(ys[i], ts[i]);
    const b747::StepInfo r = acc.finish(y_base);
    out4[0] = r.overshoot;
    out4[1] = r.rise_time;
    out4[2] = r.settling_time;
    out4[3] = r.static_error;
}
