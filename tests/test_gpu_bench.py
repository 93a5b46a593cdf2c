"""bench.py's plain run at a small size: the headline and nothing else, --steps timed steps, and --dump-outputs writing the same
lists from run to run -- and the same lists from two ranks as from one (the family's lists every rank receives)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "3", "--warmup", "1", "--mbp", "8", "--contigs", "4"]


def _line(args, cwd, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ if env is None else env, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _dump(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_plain_run_times_the_steps_and_dumps_the_same_lists_twice(tmp_path):
    outs = []
    for d in ("a", "b"):
        out = _line(["--gpus", "1"] + SMALL + ["--dump-outputs", str(tmp_path / d)], tmp_path)
        outs.append(out)
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "Gbases/s" and out["higher_is_better"] is True and out["dtype"] == "u64"
        for leg in ("cold", "nruns", "valley", "rows", "c4", "c5_like", "e2e", "cpu_baseline"):
            assert leg not in out, leg
        assert out["roofline"]["unpruned"] is None and out["roofline"]["valu"] is None and out["bloom"]["build_again_s"] is None
    a, b = _dump(tmp_path / "a"), _dump(tmp_path / "b")
    assert sorted(a) == sorted(b) and sorted(a) == sorted(f"genome{g}_{c}" for g in range(3)
                                                      for c in ("digest", "index", "h1_hi", "h1_lo", "rec", "pos"))
    for n in a:
        assert a[n].dtype == np.float64 and np.array_equal(a[n], b[n]), n
    assert sum(int(a[f"genome{g}_digest"][0]) for g in range(3)) == outs[0]["config"]["minimizers_per_step_rank0"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 1024 * 1024


def test_two_ranks_dump_the_lists_one_rank_dumps(tmp_path):
    "--gpus 2 (ranks sharing the GPU through the librccl stand-in): rank 0 writes the family's lists as they arrive after exchange 2"
    standin = os.path.join(ROOT, "tests", "rccl_standin", "librccl_standin.so")
    assert os.path.exists(standin), "tests/rccl_standin/librccl_standin.so is not built (__graft_entry__.build())"
    env = dict(os.environ, NTS_RCCL_LIB=standin, NTS_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    two = _line(["--gpus", "2"] + SMALL + ["--dump-outputs", str(tmp_path / "two")], tmp_path, env)
    one = _line(["--gpus", "1"] + SMALL + ["--dump-outputs", str(tmp_path / "one")], tmp_path)
    assert two["n_gpus"] == 2 and two["steps"] == 3 and "c4" not in two
    a, b = _dump(tmp_path / "one"), _dump(tmp_path / "two")
    assert sorted(a) == sorted(b)
    for n in a:
        assert np.array_equal(a[n], b[n]), n
    assert one["config"]["minimizers_per_step_rank0"] == two["config"]["minimizers_per_step_all_genomes"]
