/* b747_stepinfo.h -- calc_stepinfo (tools/general.py:46-61) as a streaming accumulator.
 *
 * evaluate.stepinfo reduces a recorded [T, N] series; every quantity it computes is a running reduction over
 * the samples, so the evaluation kernel (k_eval_episodes, b747_lanes.h) feeds the series one sample at a time
 * and keeps nine doubles per env instead of the history.  With L samples pushed (ys[0..L-1], ts[0..L-1]):
 *   ratio_i        (ys[i] - ys[0]) / (y_base - ys[0])      a true fp64 division: bit-equal to the torch reduction
 *   overshoot      ((max ys if y_base > 0 else min ys) - y_base) / y_base * 100; NaN if y_base == 0
 *   rise_time      ts[i] - ts[0] for the first i <= L-2 with ratio_i >= 1 - band; NaN if none
 *   settling_time  ts[i] - ts[0] for the last i <= L-1 with ratio_i <= 1 - band or ratio_i >= 1 + band; NaN if none
 *   static_error   |ys[L-1] - y_base|
 * A NaN ratio compares false in both tests, as in evaluate.stepinfo.  Host + device (tests/native/stepinfo_check.cpp
 * compiles it with g++). */
#pragma once

#ifndef B747_HD
#if defined(__HIPCC__)
#define B747_HD __host__ __device__ __forceinline__
#else
#define B747_HD inline
#endif
#endif

namespace b747 {

struct StepInfo {
    double overshoot, rise_time, settling_time, static_error;
};

struct StepInfoAcc {
    double y_base, lo, hi;        /* the command and the ratio band [1 - band, 1 + band] */
    double y0, t0;                /* first sample */
    double ymax, ymin, ylast;
    double t_rise, t_settle;      /* sample times of the rise / last out-of-band sample */
    /* bit 0: a sample was pushed; 1: a rise sample seen; 2: a sample followed it (so its index is <= L-2);
     * 3: an out-of-band sample seen */
    unsigned state;

    B747_HD void init(double y_base_, double error_band = 0.05)
    {
        y_base = y_base_;
        lo = 1 - error_band;
        hi = 1 + error_band;
        y0 = t0 = ymax = ymin = ylast = t_rise = t_settle = 0.0;
        state = 0u;
    }

    B747_HD void push(double y, double t)
    {
        if (!(state & 1u)) {
            y0 = y; t0 = t; ymax = y; ymin = y;
            state |= 1u;
        }
        /* torch.max / min propagate NaN; the series is nan_to_num'ed where it can hold one */
        ymax = (y > ymax || y != y) ? y : ymax;
        ymin = (y < ymin || y != y) ? y : ymin;
        ylast = y;
        const double ratio = (y - y0) / (y_base - y0);
        if (state & 2u) state |= 4u;
        else if (ratio >= lo) { state |= 2u; t_rise = t; }
        if (ratio <= lo || ratio >= hi) { state |= 8u; t_settle = t; }
    }

    B747_HD StepInfo finish(double y_base_) const
    {
        const double nan = __builtin_nan("");
        StepInfo r;
        const double peak = (y_base_ > 0) ? ymax : ymin;
        r.overshoot = (y_base_ != 0) ? (peak - y_base_) / y_base_ * 100 : nan;
        r.rise_time = ((state & 6u) == 6u) ? t_rise - t0 : nan;
        r.settling_time = (state & 8u) ? t_settle - t0 : nan;
        r.static_error = __builtin_fabs(ylast - y_base_);
        return r;
    }
};

}  // namespace b747
