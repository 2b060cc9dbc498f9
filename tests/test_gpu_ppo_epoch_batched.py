"""b747_ppo_epoch_batched (include/b747.h, additive under ABI 15): one PPO epoch of P learners with the
four update kernels batched over the members (the member on blockIdx.y).

The reference is b747_ppo_epoch_population -- the host loop over the members of the single-member kernels -- on clones
of the same state.  The batched kernels run the same operations on the same numbers in the same order per member, so
theta (over the whole stride), m, v, t and stats are compared with torch.equal: no tolerance.  The rollout buffers are
synthetic (a seeded CPU generator, as tests/test_gpu_ppo_update.py): the kernels only read them.

policy_stride is 8 floats above b747_policy_num_params(obs_dim) -- the smallest stride the entry point takes, as
b747_ppo_epoch_population -- and every float of a member past its 128 obs_dim + 8579 flat parameters (the packed
sections and the padding) holds a guard value that must survive."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CLIP, ENT_COEF, VF_COEF, MAX_NORM = 0.2, 0.01, 0.5, 0.5
BETA1, BETA2, EPS = 0.9, 0.999, 1e-5
LRS = [3e-4, 1e-3, 1e-4]
SEED, GUARD, NG = 17, -777.25, 64     # NG guard elements behind every buffer the call writes


def _lib_L():
    from b747_rl_ctrl_amd import _lib
    return _lib, _lib.lib()


@functools.lru_cache(maxsize=None)
def _case(od, P, n_rows, epochs):
    """P members on a shared synthetic rollout of P * n_rows rows: member p's parameters (different per member) at the
    head of its stride with guard values behind them, its perm rows (global row numbers, a permutation of its own
    rows per epoch)"""
    from b747_rl_ctrl_amd.ppo import ActorCritic
    _, L = _lib_L()
    g = torch.Generator().manual_seed(SEED + od + 31 * P + n_rows)
    torch.manual_seed(SEED + od)
    n = P * n_rows
    old = ActorCritic(od)
    with torch.no_grad():
        for prm in old.parameters():
            prm.add_(0.05 * torch.randn(prm.shape, generator=g))
        old.log_std.fill_(-0.3)
    base = old.flat_params().detach().clone()
    n_params = base.numel()
    assert n_params == 128 * od + 8579
    stride = int(L.b747_policy_num_params(od)) + 8
    theta = torch.full((P, stride), GUARD)
    for p in range(P):
        theta[p, :n_params] = base + 0.02 * torch.randn(n_params, generator=g)
    obs = torch.randn(n, od, generator=g)
    with torch.no_grad():
        mean, _ = old.double()(obs.double())
        act = (mean + old.log_std.exp() * torch.randn(n, 1, generator=g, dtype=torch.float64)).float()
        old_logp = (old.log_prob(mean, act.double()) + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).float()
    adv = 0.3 + 1.5 * torch.randn(n, generator=g)
    ret = torch.randn(n, generator=g)
    perms = torch.stack([torch.stack([p * n_rows + torch.randperm(n_rows, generator=g) for p in range(P)])
                         for _ in range(epochs)])
    dev = torch.device("cuda")
    return {"od": od, "P": P, "n_rows": n_rows, "epochs": epochs, "n_params": n_params, "stride": stride,
            "theta": theta.to(dev), "bufs": tuple(t.contiguous().to(dev) for t in (obs, act, old_logp, adv, ret)),
            "perms": perms.contiguous().to(dev), "lrs": [LRS[p % 3] * (1 + p // 3) for p in range(P)]}


class _State:
    """theta, the Adam moments, the step counts and the statistics rows of one run, each with NG guard elements behind"""

    def __init__(self, c, n_mb, members=None):
        dev = c["theta"].device
        order = list(range(c["P"])) if members is None else list(members)
        self.P, self.n_mb, self.c = len(order), n_mb, c
        P, E, n_params, stride = self.P, c["epochs"], c["n_params"], c["stride"]
        idx = torch.tensor(order, device=dev)
        self.theta = torch.full((P * stride + NG,), GUARD, device=dev)
        self.theta[:P * stride] = c["theta"][idx].reshape(-1)
        self.m = torch.full((P * n_params + NG,), GUARD, device=dev)
        self.v = torch.full((P * n_params + NG,), GUARD, device=dev)
        self.m[:P * n_params] = 0
        self.v[:P * n_params] = 0
        self.t = torch.full((P + NG,), -7, dtype=torch.int64, device=dev)
        self.t[:P] = 0
        self.stats = torch.full((E * P * n_mb * 8 + NG,), GUARD, device=dev)
        self.stats[:E * P * n_mb * 8] = float("nan")
        self.perms = torch.full((E * P * c["n_rows"] + NG,), -1, dtype=torch.int64, device=dev)
        self.perms[:E * P * c["n_rows"]] = c["perms"][:, idx].reshape(-1)
        self.perms0 = self.perms.clone()
        self.lrs = [c["lrs"][p] for p in order]

    def perm(self, e):
        n = self.P * self.c["n_rows"]
        return self.perms[e * n:(e + 1) * n]

    def stats_of(self, e):
        n = self.P * self.n_mb * 8
        return self.stats[e * n:(e + 1) * n]

    def tensors(self):
        return {"theta": self.theta, "m": self.m, "v": self.v, "t": self.t, "stats": self.stats}

    def snapshot(self):
        return {k: x.clone() for k, x in self.tensors().items()}

    def restore(self, snap):
        for k, x in self.tensors().items():
            x.copy_(snap[k])

    def check_guards(self):
        P, c = self.P, self.c
        th = self.theta[:P * c["stride"]].view(P, c["stride"])
        assert bool((th[:, c["n_params"]:] == GUARD).all()), "theta: the floats of a stride past the flat parameters"
        assert bool((self.theta[P * c["stride"]:] == GUARD).all()), "behind theta"
        assert bool((self.m[P * c["n_params"]:] == GUARD).all()) and bool((self.v[P * c["n_params"]:] == GUARD).all())
        assert bool((self.t[P:] == -7).all()), "behind t"
        assert bool((self.stats[c["epochs"] * P * self.n_mb * 8:] == GUARD).all()), "behind stats"
        assert torch.equal(self.perms, self.perms0), "perm (every row and the guard behind the last) is read only"


def _reference(c, batch, members=None, epochs=None):
    """b747_ppo_epoch_population, one call per epoch"""
    _lib, L = _lib_L()
    ptr = lambda x: x.data_ptr()
    n_mb = -(-c["n_rows"] // batch)
    st = _State(c, n_mb, members)
    dev = st.theta.device
    ws = torch.empty(int(L.b747_ppo_update_workspace(c["od"])), dtype=torch.uint8, device=dev)
    grad = torch.empty(c["n_params"], device=dev)
    lr = (ctypes.c_double * st.P)(*st.lrs)
    for e in range(c["epochs"] if epochs is None else epochs):
        _lib.check(L.b747_ppo_epoch_population(
            ptr(st.theta), st.P, c["stride"], c["od"], *(ptr(b) for b in c["bufs"]), ptr(st.perm(e)), c["n_rows"], batch,
            CLIP, ENT_COEF, VF_COEF, ptr(ws), ptr(grad), ptr(st.m), ptr(st.v), ptr(st.t), MAX_NORM, lr, BETA1, BETA2, EPS,
            ptr(st.stats_of(e)), torch.cuda.current_stream().cuda_stream), "b747_ppo_epoch_population")
    torch.cuda.synchronize()
    return st


class _Batched:
    """the state of one b747_ppo_epoch_batched run, its device learning rates and its workspace: `ws_members` slices
    (default: one per member) filled with the byte `fill`, NG guard bytes behind them"""

    def __init__(self, c, batch, members=None, ws_members=None, fill=0x5A):
        _, L = _lib_L()
        self.c, self.batch = c, batch
        self.st = _State(c, -(-c["n_rows"] // batch), members)
        dev = self.st.theta.device
        self.per = int(L.b747_ppo_epoch_batched_workspace(c["od"], batch))
        assert self.per > 0 and self.per % 16 == 0
        self.ws_bytes = (self.st.P if ws_members is None else ws_members) * self.per
        self.ws = torch.full((self.ws_bytes + NG,), 0xC3, dtype=torch.uint8, device=dev)
        self.ws[:self.ws_bytes] = fill
        self.lr = torch.tensor(self.st.lrs, dtype=torch.float64, device=dev)

    def call(self, e):
        _lib, L = _lib_L()
        ptr, c, st = (lambda x: x.data_ptr()), self.c, self.st
        _lib.check(L.b747_ppo_epoch_batched(
            ptr(st.theta), st.P, c["stride"], c["od"], *(ptr(b) for b in c["bufs"]), ptr(st.perm(e)), c["n_rows"],
            self.batch, CLIP, ENT_COEF, VF_COEF, ptr(self.ws), self.ws_bytes, ptr(st.m), ptr(st.v), ptr(st.t), MAX_NORM,
            ptr(self.lr), BETA1, BETA2, EPS, ptr(st.stats_of(e)), torch.cuda.current_stream().cuda_stream),
            "b747_ppo_epoch_batched")

    def run(self, epochs=None):
        for e in range(self.c["epochs"] if epochs is None else epochs):
            self.call(e)
        torch.cuda.synchronize()
        assert bool((self.ws[self.ws_bytes:] == 0xC3).all()), "behind the workspace"
        self.st.check_guards()
        return self.st


def _assert_same(ref, got):
    c, P = ref.c, ref.P
    n_stats = c["epochs"] * P * ref.n_mb * 8
    assert bool(torch.isfinite(ref.stats[:n_stats]).all()), "the reference wrote every statistics row"
    assert ref.t[:P].tolist() == [c["epochs"] * ref.n_mb] * P
    th0 = c["theta"][:, :c["n_params"]]
    th = ref.theta[:P * c["stride"]].view(P, c["stride"])[:, :c["n_params"]]
    assert bool(torch.isfinite(th).all())
    for name, a in ref.tensors().items():
        b = got.tensors()[name]
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} entries differ"
    return th, th0


@functools.lru_cache(maxsize=None)
def _base_reference(od):
    """P = 3, 896 rows per member, batch 256 (four minibatches, the last of 128 rows), two epochs: computed once,
    shared by the tests below, never modified"""
    return _reference(_case(od, 3, 896, 2), 256)


@pytest.mark.parametrize("od", [3, 5, 7, 8, 10])
def test_two_epochs_of_three_members_give_the_bits_of_the_member_loop(od):
    c = _case(od, 3, 896, 2)
    ref = _base_reference(od)
    ref.check_guards()
    got = _Batched(c, 256).run()
    th, th0 = _assert_same(ref, got)
    for p in range(3):                                   # different members, each updated
        assert not torch.equal(th[p], th0[p])
        for q in range(p + 1, 3):
            assert not torch.equal(th[p], th[q])
    assert len(set(c["lrs"])) == 3 and not torch.equal(c["perms"][0, 0], c["perms"][0, 1] - 896)   # (own rates, own orders)


@pytest.mark.parametrize("P,n_rows,batch", [
    (2, 6, 2),          # one tile with 30 dead lanes, three minibatches
    (2, 99, 33),        # two tiles in one workgroup
    (2, 195, 65),       # two workgroups
    (2, 16454, 16454),  # 515 tiles on the full 256-workgroup grid: three wave slots take a second tile
])
def test_edge_shapes(P, n_rows, batch):
    c = _case(3, P, n_rows, 1)
    _assert_same(_reference(c, batch), _Batched(c, batch).run())


def test_one_member():
    c = _case(3, 3, 896, 2)
    _assert_same(_reference(c, 256, members=[0]), _Batched(c, 256, members=[0]).run())


def test_a_workspace_for_two_of_three_members_runs_chunks_of_two_and_one():
    c = _case(3, 3, 896, 2)
    _assert_same(_base_reference(3), _Batched(c, 256, ws_members=2).run())


def test_a_workspace_of_nans_for_seven_members():
    c = _case(3, 3, 896, 2)
    _assert_same(_base_reference(3), _Batched(c, 256, ws_members=7, fill=0xFF).run())


def test_the_members_in_reverse_order_give_the_reversed_result():
    c = _case(3, 3, 896, 2)
    ref = _base_reference(3)
    got = _Batched(c, 256, members=[2, 1, 0]).run()
    P, stride, n_params, n_mb = 3, c["stride"], c["n_params"], ref.n_mb
    flip = lambda x, n, shape: x[:n].view(*shape).flip(shape.index(P))
    assert torch.equal(flip(got.theta, P * stride, (P, stride)), ref.theta[:P * stride].view(P, stride))
    assert torch.equal(flip(got.m, P * n_params, (P, n_params)), ref.m[:P * n_params].view(P, n_params))
    assert torch.equal(flip(got.v, P * n_params, (P, n_params)), ref.v[:P * n_params].view(P, n_params))
    assert torch.equal(got.t[:P], ref.t[:P])
    n = 2 * P * n_mb * 8
    assert torch.equal(flip(got.stats, n, (2, P, n_mb * 8)), ref.stats[:n].view(2, P, n_mb * 8))
    assert not torch.equal(got.theta, ref.theta)


def test_a_captured_graph_replayed_twice_gives_the_bits_of_two_direct_calls():
    """(every step raises at the first error: _lib.check on the entry point's return value, torch on the capture, the
    replays and the synchronisations)"""
    c = _case(3, 3, 896, 2)
    direct = _Batched(c, 256)
    direct.call(0)
    direct.call(0)                       # the same perm and statistics rows twice: what two replays do
    torch.cuda.synchronize()
    run = _Batched(c, 256)
    start = run.st.snapshot()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):  # (the capture launches nothing)
        run.call(0)
    torch.cuda.synchronize()
    run.st.restore(start)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    run.st.check_guards()
    assert direct.st.t[:3].tolist() == [8] * 3
    for name, a in direct.st.tensors().items():
        b = run.st.tensors()[name]
        same = (a == b) | (a.isnan() & b.isnan()) if a.is_floating_point() else a == b    # (epoch 1's rows: unwritten)
        assert bool(same.all()), f"{name}: {int((~same).sum())} of {a.numel()} entries differ"
