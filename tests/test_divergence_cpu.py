"""Divergence estimate without a GPU: the Mash distance of two sketches, the bottom-s merge, the CPU reference sketch on FASTA edge
cases, and `ntSynt -d auto` with the estimator stubbed -- same settings lines and the same pipeline.run arguments as the printed
value given with -d, no estimate for a command line that fails anyway, the same argparse error for a bad -d."""
import math

import numpy as np
import pytest

from ntsynt_amd import cli, divergence, pipeline, synth
from tests.divergence_ref import ref_sketch
from tests.helpers import random_records

U64 = np.uint64


def test_identical_and_disjoint_sketches():
    a = np.arange(10, 110, dtype=U64)
    assert divergence.distance(a, a, 21, 100) == (0.0, 100, 100)
    b = np.arange(1000, 1100, dtype=U64)
    assert divergence.distance(a, b, 21, 100) == (1.0, 0, 100)
    assert divergence.distance(np.zeros(0, U64), np.zeros(0, U64), 21, 100)[0] == 1.0


def test_hand_worked_jaccard():
    # A = {1..8}, B = {5..12}, s = 6: bottom-6(A u B) = {1..6}; of those 5 and 6 are in both => j = 2 / 6
    a = np.arange(1, 9, dtype=U64)
    b = np.arange(5, 13, dtype=U64)
    d, shared, size = divergence.distance(a, b, 21, 6)
    j = 2 / 6
    assert (shared, size) == (2, 6)
    assert d == pytest.approx(-math.log(2 * j / (1 + j)) / 21, rel=1e-12)
    # symmetric, and k scales it
    assert divergence.distance(b, a, 21, 6)[0] == d
    assert divergence.distance(a, b, 7, 6)[0] == pytest.approx(3 * d, rel=1e-12)


def test_merge_is_the_bottom_s_of_the_union_and_associative():
    rng = np.random.default_rng(5)
    for s in (1, 7, 50, 1000):
        x, y, z = (np.unique(rng.integers(0, 2**64 - 1, size=n, dtype=U64, endpoint=False))[:s] for n in (300, 40, 900))
        whole = np.unique(np.concatenate([x, y, z]))[:s]
        left = divergence.merge(divergence.merge(x, y, s), z, s)
        right = divergence.merge(x, divergence.merge(y, z, s), s)
        assert np.array_equal(left, whole) and np.array_equal(right, whole)
        assert left.dtype == np.uint64


def test_suggested_divergence_rounds_up_to_a_thousandth():
    assert divergence.suggested_divergence(0.0) == 0.0
    assert divergence.suggested_divergence(0.007) == 0.7            # exact values stay
    assert divergence.suggested_divergence(0.0070001) == 0.701
    assert divergence.suggested_divergence(0.125) == 12.5
    assert divergence.suggested_divergence(1.0) == 100.0
    for d in np.random.default_rng(1).random(200) * 0.3:
        v = divergence.suggested_divergence(float(d))
        assert float(str(v)) == v and 100 * d <= v + 1e-9 and v - 100 * d < 0.001 + 1e-9


def test_reference_sketch_edge_cases():
    rng = np.random.default_rng(9)
    k = 21
    seqs = random_records(rng, [5000, 15, 0, 20, 3000, 21], n_frac=0.05, lower_frac=0.1)
    full = ref_sketch(seqs, k, 10**6)
    assert full.size > 0 and np.all(np.diff(full.astype(object)) > 0)
    # records shorter than k add nothing; the sketch of the records merges from the sketches of the parts
    assert np.array_equal(ref_sketch([q for q in seqs if len(q) >= k], k, 10**6), full)
    for s in (1, 100, 2000):
        assert np.array_equal(ref_sketch(seqs, k, s), full[:s])
        parts = [ref_sketch(seqs[:3], k, s), ref_sketch(seqs[3:], k, s)]
        assert np.array_equal(divergence.merge(parts[0], parts[1], s), full[:s])
    # lower case is the same k-mer
    up = [bytes(np.frombuffer(q, np.uint8) & np.uint8(0xDF)) if q else q for q in seqs]
    assert np.array_equal(ref_sketch(up, k, 10**6), full)
    # fewer distinct k-mers than s: a tandem array of one 7-mer unit has 7 distinct 21-mers (fewer canonical ones at most)
    unit = b"ACGTTGC" * 200
    assert 1 <= ref_sketch([unit], k, 10000).size <= 7


def test_mash_distance_of_cpu_sketches_tracks_the_substitution_rate():
    "relatives with per-genome substitution rate r differ at p = 2r(1 - r) + 2r^2/3; D estimates -ln(1 - p)"
    anc = synth.make_ancestor(400_000, 2, seed=3)
    for p_target in (0.01, 0.03):
        gs = [synth.derive_genome(anc, p_target, j, seed=3, structural=False) for j in range(2)]
        p = float(np.mean(np.concatenate(gs[0]) != np.concatenate(gs[1])))
        sk = [ref_sketch([c.tobytes() for c in g], 21, 5000) for g in gs]
        d = divergence.distance(sk[0], sk[1], 21, 5000)[0]
        expect = -math.log(1 - p)
        assert abs(d - expect) <= 0.1 * expect + 2e-4, (d, expect)


# ---- ntSynt -d auto ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fastas(tmp_path):
    paths = []
    for i in range(3):
        p = tmp_path / f"g{i}.fa"
        p.write_text(">a\nACGT\n")
        paths.append(str(p))
    return paths


def _stub_estimate(value, calls):
    def estimate(paths, k=21, s=10000, device=0, ctx=None):
        calls.append((list(paths), k, s, device))
        est = divergence.Estimate(names=list(paths), k=k, s=s, divergence=value, largest=(0, len(paths) - 1))
        return est
    return estimate


def _run_cli(monkeypatch, capsys, argv):
    seen = []
    # (the log callable is a fresh lambda per run: compared by what it is)
    monkeypatch.setattr(pipeline, "run", lambda *a, **kw: seen.append((a, dict(kw, log=kw["log"] is print))))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    rc = cli.main(argv)
    return rc, capsys.readouterr().out, seen


@pytest.mark.parametrize("value", [0.7, 12.5, 3.127])
@pytest.mark.parametrize("dry", [False, True])
def test_auto_runs_exactly_as_the_printed_value(monkeypatch, capsys, fastas, value, dry):
    calls = []
    monkeypatch.setattr(divergence, "estimate", _stub_estimate(value, calls))
    extra = ["-n"] if dry else []
    rc_a, out_a, seen_a = _run_cli(monkeypatch, capsys, fastas + ["-d", "auto", "-p", "x"] + extra)
    assert len(calls) == 1 and calls[0] == (fastas, 21, 10000, 0)
    first, rest = out_a.split("\n", 1)
    assert first == f"Estimated percent divergence: {value} (largest pair: {fastas[0]} vs {fastas[2]}; k 21, sketch 10000)"
    printed = first.split()[3]
    rc_n, out_n, seen_n = _run_cli(monkeypatch, capsys, fastas + ["-d", printed, "-p", "x"] + extra)
    assert len(calls) == 1                                            # a numeric -d estimates nothing
    assert rc_a == rc_n == 0 and rest == out_n
    assert f"\t--divergence {value}\n" in out_n
    assert seen_a == seen_n and len(seen_a) == (0 if dry else 1)


def test_auto_selects_the_row_of_the_printed_value(monkeypatch, capsys, fastas):
    for value, row in ((0.7, (500, 10000, 10000)), (3.0, (1000, 100000, 50000)), (12.5, (10000, 1000000, 100000))):
        monkeypatch.setattr(divergence, "estimate", _stub_estimate(value, []))
        _, _, seen = _run_cli(monkeypatch, capsys, fastas + ["-d", "auto"])
        kw = seen[0][1]
        assert (kw["block_size"], int(kw["merge"]), kw["indel"]) == row


def test_auto_with_fastas_list(monkeypatch, capsys, fastas, tmp_path):
    calls = []
    monkeypatch.setattr(divergence, "estimate", _stub_estimate(1.5, calls))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(fastas) + "\n")
    _run_cli(monkeypatch, capsys, ["--fastas_list", str(lst), "-d", "auto", "-n"])
    assert calls[0][0] == fastas


@pytest.mark.parametrize("case", ["one", "both", "none", "missing"])
def test_no_estimate_for_a_command_line_that_fails_anyway(monkeypatch, capsys, fastas, tmp_path, case):
    calls = []
    monkeypatch.setattr(divergence, "estimate", _stub_estimate(1.0, calls))
    monkeypatch.setattr(pipeline, "run", lambda *a, **kw: None)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(fastas) + "\n")
    argv = {"one": fastas[:1], "both": fastas[:2] + ["--fastas_list", str(lst)], "none": [],
            "missing": fastas[:2] + [str(tmp_path / "nope.fa")]}[case] + ["-d", "auto"]
    if case == "missing":
        with pytest.raises(FileNotFoundError, match="nope.fa not found"):
            cli.main(argv)
    else:
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
    assert calls == []


@pytest.mark.parametrize("bad", ["abc", "a.fa", "Auto", ""])
def test_bad_divergence_value_gives_the_argparse_error_of_before(capsys, bad):
    with pytest.raises(SystemExit) as e:
        cli.main(["a.fa", "b.fa", "-d", bad])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert err.rstrip().endswith(f"argument -d/--divergence: invalid float value: {bad!r}")


def test_divergence_launcher_refuses_before_the_gpu(capsys, tmp_path):
    from ntsynt_amd import stage_cli
    with pytest.raises(SystemExit) as e:
        stage_cli.ntsynt_divergence([str(tmp_path / "a.fa")])
    assert e.value.code == 2
    with pytest.raises(FileNotFoundError):
        stage_cli.ntsynt_divergence([str(tmp_path / "a.fa"), str(tmp_path / "b.fa")])


def test_estimate_table_text():
    sk = [np.arange(0, 100, dtype=U64), np.arange(10, 110, dtype=U64), np.arange(50, 150, dtype=U64)]
    est = divergence.from_sketches(["a.fa", "b.fa", "c.fa"], sk, 21, 100)
    lines = est.table().splitlines()
    assert lines[0] == "genome_a\tgenome_b\tdistance\tshared_hashes\tsketch_size"
    assert [ln.split("\t")[:2] for ln in lines[1:4]] == [["a.fa", "b.fa"], ["a.fa", "c.fa"], ["b.fa", "c.fa"]]
    d_ac = divergence.distance(sk[0], sk[2], 21, 100)[0]
    assert est.largest == (0, 2) and lines[2].split("\t")[3:] == ["50", "100"]
    assert lines[4] == f"# ntSynt -d {divergence.suggested_divergence(d_ac)}"
