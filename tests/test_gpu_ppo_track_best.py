"""b747_ppo_track_best alone (include/b747.h) against the NumPy transcription of the reference's
ControlTestCallback (tests/control_test_ref.py).

40 calls with repeats cycling 1, 2, 1, 3 (70 pushes: the ring wraps for W = 30 and W = 5, and repeats straddle the wrap)
on hand-made evaluation results: P = 3 (and P = 1) members, R = 4 reported envs of 64, n_eval = (P - 1) * 64 + 4.
  member 0  quality rises all the way: it saves at every call
  member 1  NaN ITSE in the first calls, finite afterwards: no save while a NaN is in the window; its settling time is
            NaN in some calls
  member 2  the windowed quality peaks at call 6 and declines: the snapshot stays call 6's while params keeps changing
Envs 4 .. 63 of every group hold NaN and 1e300, so reading one of them shows.  params is rewritten before every call with
values that encode (call, member, index); best_params has one row more than members, which must survive.

The reference is driven from the kernel's own `last`, read back: from there window_mean, best_quality, best_eval, count,
the ring and best_params are exact (==, NaN positions equal).  last's settling-time and overshoot columns are exact
against np.mean; its quality column is held to 4 ulp of NumPy's value (the device library documents its double exp at
1 ulp, as NumPy's is; the mean of four such values adds at most one rounding each).  The reference's own margins
|window_mean.quality - best so far| at every decision must exceed 1e-9, so a 4-ulp difference cannot flip a save and an
input that made a decision marginal fails here instead of hiding."""
import math

import numpy as np
import pytest
import torch

import control_test_ref as R

pytestmark = pytest.mark.gpu

CALLS, REPEATS, NREF, EPP, TK = 40, (1, 2, 1, 3), 4, 64, 20.0
REFS = [math.radians(v) for v in (5.0, -5.0, 10.0, -10.0)]


def _target_quality(call, member):
    if member == 0:
        return 0.2 + 0.015 * call
    if member == 1:
        return math.nan if call < 3 else 0.5 + 0.2 * math.sin(call)
    return 0.3 + 0.05 * call if call <= 6 else 0.1 - 0.001 * (call - 7)


def _inputs(P):
    """eval_out [CALLS, 7, n] and vref [n] (float64, CPU)"""
    n = (P - 1) * EPP + NREF
    out = np.empty((CALLS, 7, n))
    out[:, :, 0::2], out[:, :, 1::2] = np.nan, 1e300
    vref = np.full(n, np.nan)
    for p in range(P):
        for r in range(NREF):
            i = p * EPP + r
            vref[i] = REFS[r]
            for c in range(CALLS):
                q = _target_quality(c, p)
                itse = math.nan if q != q else -math.log(q) * TK * REFS[r] ** 2 / 6 * (1 + 0.01 * r)
                out[c, :, i] = 0.25 * c + r + p             # rows nobody reads
                out[c, 4, i] = itse
                out[c, 2, i] = math.nan if (p == 1 and c % 7 == 3 and r == 2) else 3.0 + 0.1 * c + 0.01 * r + p
                out[c, 0, i] = (-1) ** (r + c) * (5.0 + 0.3 * c + r + 0.1 * p)
    return out, vref


def _params(call, P, stride):
    idx = torch.arange(stride, dtype=torch.float32)[None] % 97
    return (call * 1000 + torch.arange(P, dtype=torch.float32)[:, None] * 100 + idx).contiguous()


@pytest.mark.parametrize("extra", [0, 8], ids=["stride", "stride+8"])
@pytest.mark.parametrize("W", [30, 5])
@pytest.mark.parametrize("P", [3, 1])
def test_the_kernel_keeps_the_callbacks_books(P, W, extra):
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda")
    stride = int(L.b747_policy_num_params(3)) + extra
    n = (P - 1) * EPP + NREF
    ev_np, vref_np = _inputs(P)
    ev, vref = torch.from_numpy(ev_np).to(dev), torch.from_numpy(vref_np).to(dev)
    f64 = torch.float64
    ring = torch.full((3, P, W), math.nan, dtype=f64, device=dev)
    count = torch.zeros(P, dtype=torch.int64, device=dev)
    last, wmean = torch.full((P, 3), math.nan, dtype=f64, device=dev), torch.full((P, 3), math.nan, dtype=f64, device=dev)
    best_q = torch.zeros(P, dtype=f64, device=dev)
    best_e = torch.full((P,), -1, dtype=torch.int64, device=dev)
    best_p = torch.full((P + 1, stride), -1.0, dtype=torch.float32, device=dev)
    params = torch.zeros(P, stride, dtype=torch.float32, device=dev)
    log = {k: [] for k in ("last", "window_mean", "best_quality", "best_eval", "count", "best_params")}
    p_ = torch.Tensor.data_ptr
    repeats = [REPEATS[c % 4] for c in range(CALLS)]
    for c in range(CALLS):
        params.copy_(_params(c, P, stride))
        _lib.check(L.b747_ppo_track_best(p_(ev[c]), n, p_(vref), TK, P, EPP, NREF, W, repeats[c], p_(params), stride,
                                         p_(ring), p_(count), p_(last), p_(wmean), p_(best_q), p_(best_e), p_(best_p),
                                         torch.cuda.current_stream().cuda_stream), "b747_ppo_track_best")
        for k, t in (("last", last), ("window_mean", wmean), ("best_quality", best_q), ("best_eval", best_e),
                     ("count", count), ("best_params", best_p)):
            log[k].append(t.clone())
    got = {k: torch.stack(v).cpu().numpy() for k, v in log.items()}       # one synchronisation
    ring_got = ring.cpu().numpy()

    # ---- last: the means over the four reported envs
    sel = np.array([[p * EPP + r for r in range(NREF)] for p in range(P)])
    for c in range(CALLS):
        st, ov, it = ev_np[c, 2][sel], np.abs(ev_np[c, 0][sel]), ev_np[c, 4][sel]
        want = R.means([st.tolist(), ov.tolist(), R.quality(it, vref_np[sel], TK).tolist()])
        assert R.same(got["last"][c][:, :2], want[:, :2]), (c, got["last"][c], want)
        q, wq = got["last"][c][:, 2], want[:, 2]
        assert np.array_equal(q != q, wq != wq), (c, q, wq)
        ok = wq == wq
        ulps = np.abs(q[ok] - wq[ok]) / np.spacing(wq[ok])
        print(f"call {c}: quality {q} against NumPy {wq}: {ulps} ulp")
        assert np.all(ulps <= 4), (c, q, wq, ulps)

    # ---- everything downstream of last: exact
    ref = R.track(list(got["last"]), repeats, W)
    saved_at = [-1] * P
    for c, want in enumerate(ref):
        decided = want["margin"][np.isfinite(want["margin"])]
        assert np.all(decided > 1e-9), (c, want["margin"])
        for k in ("window_mean", "best_quality", "best_eval", "count"):
            assert R.same(got[k][c], want[k]), (c, k, got[k][c], want[k])
        for p in range(P):
            if want["saved"][p]:
                saved_at[p] = c
            row = _params(saved_at[p], 1, stride)[0].numpy() + 100 * p if saved_at[p] >= 0 else np.full(stride, -1.0)
            assert np.array_equal(got["best_params"][c][p], row), (c, p, saved_at[p])
        assert np.all(got["best_params"][c][P] == -1.0), (c, "the row behind the members was written")
    assert R.same(ring_got, R.ring(list(got["last"]), repeats, W))

    # ---- the scenario is the one the docstring describes
    saves = np.array([w["saved"] for w in ref])
    assert saves[:, 0].all()
    if P == 3:
        assert not saves[:3, 1].any() and saves[:, 1].any()
        first = int(np.argmax(saves[:, 1]))
        nan_pushes = sum(repeats[:3])
        # the NaN entries have to leave the window first: it holds the pushes [count - W, count)
        assert sum(repeats[:first]) < nan_pushes + W <= sum(repeats[:first + 1])
        assert np.isnan(got["window_mean"][:first, 1, 2]).all()
        assert np.isnan(got["last"][3, 1, 0]) and np.isnan(got["window_mean"][3, 1, 0])
        assert saves[:7, 2].all() and not saves[7:, 2].any() and saved_at[2] == 6
        assert int(got["best_eval"][-1][2]) == sum(repeats[:7]) - 1
    assert got["count"][-1].tolist() == [sum(repeats)] * P
