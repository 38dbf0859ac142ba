"""bench.py on the device: a plain run prints the headline line only and --dump-outputs writes what
the timed steps computed (one short run of the smallest workload, shared by the tests)."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("bench") / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "mt10_w400", "--settle-s", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=120)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout, p.stderr[-2000:])
    return json.loads(lines[0]), out


def test_plain_run_prints_the_headline_line_only(plain_run):
    d, _ = plain_run
    assert d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "SAC gradient-steps/sec" and d["dtype"].startswith("fp32")
    assert d["value"] > 0 and d["ms_per_step"] == pytest.approx(1e3 / d["value"])
    for k in ("roofline", "gemm_families", "gemm_kernel_ms_per_step", "cpu_baseline"):  # --full only
        assert k not in d


def test_dump_outputs_holds_the_logs_and_the_stepped_networks(plain_run):
    from mtrl_amd import _lib as L
    from mtrl_amd.init import init_mtsac

    d, out = plain_run
    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(arrays) == ["actor", "critic", "critic_target", "log_alpha", "logs"]
    assert all(a.dtype in (np.float32, np.float64) and a.ndim == 1 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["logs"].tolist() == [d["logs"][k] for k in L.LOG_KEYS]
    # MT10 / W400 stays under the sampling cap: the whole networks, three Adam steps away from the seeded
    # init (a step moves a weight by at most lr (1 - b1) / sqrt(1 - b2) = 3.2 lr), the target behind the critic
    from mtrl_amd.engine import default_config

    c = default_config(10)
    actor, critic = init_mtsac(10, 49, 4, 400, 3, 400, 3, 2, seed=1)
    for got, init, lr in ((arrays["actor"], actor, c.actor_lr), (arrays["critic"], critic, c.critic_lr)):
        assert got.shape == init.shape
        moved = np.abs(got - init).max()
        assert 0 < moved <= 3 * 3.2 * lr, (moved, lr)
    assert arrays["critic_target"].shape == critic.shape
    assert 0 < np.abs(arrays["critic_target"] - critic).max() < np.abs(arrays["critic"] - critic).max()
    assert arrays["log_alpha"].shape == (10,)
