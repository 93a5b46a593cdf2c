"""bench.py's command line and its --dump-outputs format, on the host: what the options parse to, and that the files written for a
minimizer list are float64, exact, the same from call to call, and within the size the option promises."""
import os
import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_steps_must_be_timed(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def _lists(seed, sizes):
    rng = np.random.default_rng(seed)
    out = []
    for g, n in enumerate(sizes):
        h1 = rng.integers(0, np.iinfo(np.uint64).max, size=n, dtype=np.uint64, endpoint=True)
        rec = np.sort(rng.integers(0, 24, size=n)).astype(np.uint32)
        pos = rng.integers(0, 3_000_000_000 // 24, size=n).astype(np.uint64)
        out.append((f"genome{g}", (h1, rec, pos)))
    return out


def test_dump_is_float64_exact_and_repeatable(tmp_path):
    lists = _lists(5, [5000, 300, 0])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), lists, sample=3000)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert names == sorted(f"genome{g}_{c}.npy" for g in range(3) for c in ("digest", "index", "h1_hi", "h1_lo", "rec", "pos"))
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and np.array_equal(a, b), n
    for name, (h1, rec, pos) in lists:
        f = {c: np.load(tmp_path / "a" / f"{name}_{c}.npy") for c in ("digest", "index", "h1_hi", "h1_lo", "rec", "pos")}
        idx = f["index"].astype(np.int64)
        assert idx.size == min(h1.size, 1000) and np.all(np.diff(idx) > 0)          # (3000 over three lists; the small ones whole)
        h = (f["h1_hi"].astype(np.uint64) << np.uint64(32)) | f["h1_lo"].astype(np.uint64)
        assert np.array_equal(h, h1[idx]) and np.array_equal(f["rec"].astype(np.uint32), rec[idx])
        assert np.array_equal(f["pos"].astype(np.uint64), pos[idx])
        dg = bench.mx_digest(h1, rec, pos)
        d = f["digest"].astype(np.uint64)
        assert int(d[0]) == dg["n"] and (int(d[1]) << 32 | int(d[2])) == dg["xor_h1"] and (int(d[3]) << 32 | int(d[4])) == dg["sum_mix"]


def test_dump_sees_a_changed_minimizer_outside_its_sample(tmp_path):
    "the digest covers the whole list, the sample a part of it"
    lists = _lists(6, [4000])
    bench.dump_outputs(str(tmp_path / "a"), lists, sample=100)
    idx = set(np.load(tmp_path / "a" / "genome0_index.npy").astype(np.int64).tolist())
    j = next(i for i in range(4000) if i not in idx)
    h1, rec, pos = lists[0][1]
    h1 = h1.copy()
    h1[j] ^= np.uint64(1)
    bench.dump_outputs(str(tmp_path / "b"), [("genome0", (h1, rec, pos))], sample=100)
    assert np.array_equal(np.load(tmp_path / "a" / "genome0_h1_lo.npy"), np.load(tmp_path / "b" / "genome0_h1_lo.npy"))
    assert not np.array_equal(np.load(tmp_path / "a" / "genome0_digest.npy"), np.load(tmp_path / "b" / "genome0_digest.npy"))


def test_dump_stays_within_64_MB(tmp_path):
    "eight lists (config 4's family) longer than the sample together: what lands on disk"
    bench.dump_outputs(str(tmp_path), _lists(7, [200_000] * 8))
    total = sum(os.path.getsize(tmp_path / n) for n in os.listdir(tmp_path))
    assert bench.DUMP_SAMPLE * 5 * 8 <= total <= 64 * 1024 * 1024
