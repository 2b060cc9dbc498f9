"""tests/golden/dispatch_parent.json: the kernel b747_env_kernel reports for every row of the dispatch sweep, recorded
from a library built from the commit BEFORE the launch plans (csrc/b747_dispatch.h) replaced the hand-written dispatch.
tests/test_dispatch_plan.py runs the same sweep (sweep() below) on the current library and compares, so the expected
values never come from the code under test.  b747_env_kernel launches nothing; no GPU is needed.

Usage:  B747_LIB_PATH=/path/to/the/parent/commit's/libb747.so python tests/golden/make_dispatch_parent.py
"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "dispatch_parent.json")

COLUMNS = ("sig", "default_consts", "spec", "config", "variant", "n_env_steps", "n_sub")
# the training configuration and four single-field departures from it (field, value, obs_dim)
CONFIGS = {"training": None, "obs_speed_mode": ("obs_type", 1, 5), "use_limiter": ("use_limiter", 1, 3),
           "no_auto_reset": ("auto_reset", 0, 3), "aero_fixed": ("aero_fixed", 1, 3)}
VARIANTS = {"FAST": 0, "FAITHFUL": 1, "MIXED": 2}
PTR = 0x1000   # b747_env_kernel checks the descriptor's pointers for NULL and reads none of them


def training_config(_lib, n_sub):
    """b747_env_config_default(PID_LIKE, CLASSIC) with the AERO disturbance: main.py's configuration"""
    cfg = _lib.EnvConfig()
    assert _lib.lib().b747_env_config_default(ctypes.byref(cfg), 0, 0) == 0
    cfg.disturbance_mode = 0
    cfg.n_sub = n_sub
    return cfg


def env_batch(_lib, n, obs_dim, variant, sig, x_f64=1):
    b = _lib.EnvBatch()
    b.n, b.x_f64, b.obs_dim, b.variant = n, x_f64, obs_dim, variant
    for f in _lib._ENV_PTRS:
        setattr(b, f, PTR)
    b.sig = PTR if sig else None
    return b


def sweep(_lib):
    """[(row, kernel code)] over the full product of COLUMNS; restores b747_set_specialization"""
    L = _lib.lib()
    rows = []
    prev = L.b747_set_specialization(1)
    try:
        for sig, defc, spec, config, variant, n_env_steps, n_sub in itertools.product(
                (0, 1), (1, 0), (0, 1, 2), CONFIGS, VARIANTS, (1, 7), (1, 5)):
            L.b747_set_specialization(spec)
            cfg = training_config(_lib, n_sub)
            obs_dim = 3
            if CONFIGS[config]:
                field, value, obs_dim = CONFIGS[config]
                setattr(cfg, field, value)
            c = _lib.default_consts()
            if not defc:
                c.m0 = c.m0 + 1.0
            b = env_batch(_lib, 4096, obs_dim, VARIANTS[variant], sig)
            code = L.b747_env_kernel(ctypes.byref(b), ctypes.byref(cfg), ctypes.byref(c), n_env_steps)
            rows.append(([sig, defc, spec, config, variant, n_env_steps, n_sub], code))
    finally:
        L.b747_set_specialization(prev)
    return rows


if __name__ == "__main__":
    if not os.environ.get("B747_LIB_PATH"):
        sys.exit("B747_LIB_PATH must name the parent commit's libb747.so (see the module docstring)")
    sys.path.insert(0, ROOT)
    from b747_rl_ctrl_amd import _lib
    rows = sweep(_lib)
    with open(OUT, "w") as f:
        f.write('{"columns": %s,\n "rows": [\n' % json.dumps(list(COLUMNS) + ["kernel"]))
        f.write(",\n".join("  " + json.dumps(r + [code]) for r, code in rows))
        f.write("\n]}\n")
    print(f"{OUT}: {len(rows)} rows, kernels {sorted(set(code for _, code in rows))}")
