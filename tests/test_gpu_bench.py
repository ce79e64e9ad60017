"""bench.py end to end, on a small shape: a plain run prints the headline and leaves every leg of its own to --full;
with --full those legs run.  Both runs time the same steps on the same inputs, so their lnL and dumped arrays agree."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libpll_ref.so")
# fields only --full fills (c4_strong needs the default 1,000,000-site workload or N > 1 as well)
FULL_ONLY = ("per_step_ms", "roofline", "api_calls", "kernels", "varying_lists", "cpu_baseline",
             "lnl_rel_err_vs_reference", "c4_strong")


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_plain_and_full(gpu, tmp_path):
    shape = ["--sites", "20000", "--steps", "3", "--warmup", "1"]
    plain = _bench(shape + ["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(shape + ["--full", "--cpu-sites", "5000", "--cpu-reps", "3", "--dump-outputs", str(tmp_path / "full")])
    assert plain["full"] is False and full["full"] is True
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup_flag", "config"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert all(plain[k] is None for k in FULL_ONLY)
    for k in ("per_step_ms", "roofline", "api_calls", "kernels", "varying_lists"):
        assert full[k], k
    if os.path.exists(REF):
        assert full["cpu_baseline"]["value"] > 0 and full["lnl_rel_err_vs_reference"] < 1e-12
    assert full["c4_strong"] is None
    assert abs(plain["lnl"] - full["lnl"]) <= 1e-12 * abs(plain["lnl"])
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and "lnl.npy" in names
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.shape == b.shape and np.allclose(a, b, rtol=1e-12, atol=0), n
