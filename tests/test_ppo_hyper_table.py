"""ppo.hyper_table: the [P, 8] float64 table of per-member PPO hyper-parameters that
PopulationPPO(hyper=...) hands to b747_ppo_gae_population and the two *_hyper epoch calls.  A pure function: no env, no
GPU, no library."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("learning_rate", "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "gamma", "gae_lambda")


def _cfg():
    from b747_rl_ctrl_amd.ppo import PPOConfig
    return PPOConfig(n_steps=14, gamma=0.97, gae_lambda=0.9, clip_range=0.25, ent_coef=0.02, vf_coef=0.4,
                     max_grad_norm=0.7, learning_rate=2e-4, n_epochs=2, batch_size=256)


def test_defaults_come_from_cfg_in_the_column_order_of_the_header():
    from b747_rl_ctrl_amd.ppo import HYPER_COLS, hyper_table
    c = _cfg()
    for hyper in (None, [{}, {}, {}]):
        t = hyper_table(c, 3, hyper)
        assert t.dtype == torch.float64 and t.device.type == "cpu" and tuple(t.shape) == (3, 8) and HYPER_COLS == 8
        assert t.is_contiguous() and t.stride(0) * t.element_size() == 64
        want = [c.learning_rate, c.clip_range, c.ent_coef, c.vf_coef, c.max_grad_norm, c.gamma, c.gae_lambda, 0.0]
        assert t.tolist() == [want] * 3


def test_every_key_lands_in_its_own_column_of_its_own_row():
    from b747_rl_ctrl_amd.ppo import hyper_table
    c = _cfg()
    base = hyper_table(c, 3)
    values = dict(learning_rate=1e-3, clip_range=0.1, ent_coef=0.0, vf_coef=0.25, max_grad_norm=10.0, gamma=0.9,
                  gae_lambda=0.6)
    for col, key in enumerate(KEYS):
        t = hyper_table(c, 3, [{}, {key: values[key]}, {}])
        want = base.clone()
        want[1, col] = values[key]
        assert torch.equal(t, want), key
    t = hyper_table(c, 2, [dict(values), {}])
    assert t[0].tolist() == [values[k] for k in KEYS] + [0.0] and torch.equal(t[1], base[0])
    assert bool((t[:, 7] == 0).all())


def test_learning_rates_fill_the_rows_that_name_none():
    from b747_rl_ctrl_amd.ppo import hyper_table
    c = _cfg()
    t = hyper_table(c, 3, None, learning_rates=[3e-4, 1e-3, 1e-4])
    assert t[:, 0].tolist() == [3e-4, 1e-3, 1e-4] and t[:, 1].tolist() == [c.clip_range] * 3
    t = hyper_table(c, 3, [{"gamma": 0.9}, {}, {"vf_coef": 0.6}], learning_rates=[3e-4, 1e-3, 1e-4])
    assert t[:, 0].tolist() == [3e-4, 1e-3, 1e-4] and t[:, 5].tolist() == [0.9, c.gamma, c.gamma]
    assert t[:, 3].tolist() == [c.vf_coef, c.vf_coef, 0.6]


def test_edge_values_that_are_allowed():
    from b747_rl_ctrl_amd.ppo import hyper_table
    t = hyper_table(_cfg(), 2, [dict(gamma=0.0, gae_lambda=1.0, ent_coef=0.0, vf_coef=0.0),
                                dict(gamma=1.0, gae_lambda=0.0, max_grad_norm=1e9)])
    assert t[:, 5].tolist() == [0.0, 1.0] and t[:, 6].tolist() == [1.0, 0.0]


@pytest.mark.parametrize("kw,word", [
    (dict(hyper=[{"gama": 0.9}, {}, {}]), "gama"),
    (dict(hyper=[{"n_steps": 8}, {}, {}]), "n_steps"),
    (dict(hyper=[{"batch_size": 64}, {}, {}]), "batch_size"),
    (dict(hyper=[{}, {}]), "one entry per member"),
    (dict(hyper=[{}, {}, {}, {}]), "one entry per member"),
    (dict(learning_rates=[1e-3, 1e-3]), "one entry per member"),
    (dict(hyper=[{"learning_rate": 1e-3}, {}, {}], learning_rates=[1e-3] * 3), "learning_rates"),
    (dict(hyper=[{}, {"gamma": float("nan")}, {}]), "gamma"),
    (dict(hyper=[{}, {"learning_rate": float("inf")}, {}]), "learning_rate"),
    (dict(learning_rates=[1e-3, float("nan"), 1e-3]), "learning_rate"),
    (dict(hyper=[{}, {}, {"gamma": 1.0001}]), "gamma"),
    (dict(hyper=[{}, {}, {"gamma": -0.1}]), "gamma"),
    (dict(hyper=[{}, {}, {"gae_lambda": 1.5}]), "gae_lambda"),
    (dict(hyper=[{}, {}, {"gae_lambda": -1e-9}]), "gae_lambda"),
    (dict(hyper=[{"clip_range": 0.0}, {}, {}]), "clip_range"),
    (dict(hyper=[{"clip_range": -0.2}, {}, {}]), "clip_range"),
    (dict(hyper=[{"learning_rate": 0.0}, {}, {}]), "learning_rate"),
    (dict(learning_rates=[1e-3, 1e-3, -1e-3]), "learning_rate"),
    (dict(hyper=[{"max_grad_norm": 0.0}, {}, {}]), "max_grad_norm"),
    (dict(hyper=[{"ent_coef": -0.01}, {}, {}]), "ent_coef"),
    (dict(hyper=[{"vf_coef": -0.5}, {}, {}]), "vf_coef"),
    (dict(hyper=[{"vf_coef": float("-inf")}, {}, {}]), "vf_coef"),
])
def test_what_is_refused(kw, word):
    from b747_rl_ctrl_amd.ppo import hyper_table
    with pytest.raises(ValueError, match=word):
        hyper_table(_cfg(), 3, **kw)


def test_cfg_values_are_validated_too():
    from b747_rl_ctrl_amd.ppo import PPOConfig, hyper_table
    with pytest.raises(ValueError, match="gamma"):
        hyper_table(PPOConfig(gamma=1.5), 2)
    with pytest.raises(ValueError, match="member"):
        hyper_table(PPOConfig(), 0)


@pytest.mark.parametrize("g,l", [(0.99, 0.95), (0.9, 0.6), (0.7, 1.0), (0.97, 0.9), (1.0, 1.0), (0.9, 0.0),
                                 (0.995, 0.92), (1 / 3, 0.1)])
def test_the_documented_rounding_of_gl_is_torchs(g, l):
    """gl = (float)(gamma * gae_lambda): the fp64 product rounded to fp32 once -- what torch does with the Python
    product `gamma * gae_lambda` when it multiplies a float32 tensor by it (PPO.compute_gae's loop), and what the
    population GAE kernel computes from the table's two doubles.  g = (float)gamma likewise."""
    import struct
    gl = torch.tensor(g * l, dtype=torch.float64).float()
    once = struct.unpack("f", struct.pack("f", g * l))[0]                # IEEE round-to-nearest of the double product
    assert float(gl) == once
    x = torch.tensor([1.0, 3.0, -7.25, 1e-3], dtype=torch.float32)
    assert torch.equal((g * l) * x, gl * x)                              # torch's scalar multiply rounds the same way
    assert torch.equal(g * x, torch.tensor(g, dtype=torch.float64).float() * x)
    two = float(torch.tensor(g, dtype=torch.float64).float() * torch.tensor(l, dtype=torch.float64).float())
    assert math.isclose(two, once, rel_tol=1e-6)                         # (the two-rounding product is another number)
