"""`ntSynt --block-paf --paf-cs` and `bin/ntsynt_block_stats --paf-out F --paf-cs` end to end (ntsynt_amd/assess.py block_alignments with cs;
docs/design/04_26_block_paf_cs.md) on the family of tests/test_gpu_block_paf.py.  One run with --block-paf --paf-cs --identity-max-edits
1023 --block-ends --ends-max-len 1500 and one with the same switches less --paf-cs.  For every record tests/cs_brute.apply_cs on the
target substring read from the FASTA file gives the query substring (reverse-complemented for `-`), and cigar_of_cs gives the record's
own cg; the planted 40-base deletion appears as `-` tokens of exactly 40 target bases, each the target's own; with the cs:Z: column cut the file is that of
the run without --paf-cs, and every other file is byte-equal; the tool reproduces the file; --paf-cs without --block-paf and under
several ranks are parser errors.  Every test runs under a time limit of its own."""
import faulthandler
import os
import subprocess
import sys

import pytest

from ntsynt_amd import assess
from tests import cs_brute as CS
from tests.test_gpu_block_end_variants import PARAMS
from tests.test_gpu_block_paf import INDELS, paf_family, read_fasta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
SWITCHES = ["--block-paf", "--identity-max-edits", "1023", "--block-ends", "--ends-max-len", "1500", "--benchmark"]


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _run(cmd, cwd, **env):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT, **env))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family and two runs: --block-paf with --paf-cs and without"
    tmp = tmp_path_factory.mktemp("paf_cs_runs")
    paths, _ = paf_family(str(tmp))
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    dirs = {}
    for name, extra in (("cs", SWITCHES + ["--paf-cs"]), ("plain", SWITCHES)):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = _run(ntsynt + paths + PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, paths, dirs


def records_of(text):
    out = []
    for line in text.splitlines():
        f = line.split("\t")
        assert len(f) == 19 and [t[:5] for t in f[12:]] == list(assess.PAF_TAGS_CS), line[:200]
        out.append(dict(q=f[0], q_from=int(f[2]), q_to=int(f[3]), sign=f[4], t=f[5], t_from=int(f[7]), t_to=int(f[8]), tg=f[14][5:], qg=f[15][5:],
                        cg=f[17][5:], cs=f[18][5:]))
    return out


def test_every_record_rebuilds_its_query_and_its_cigar(runs):
    _, paths, dirs = runs
    genomes = {os.path.basename(p): {k: v.tobytes().decode() for k, v in read_fasta(p).items()} for p in paths}
    records = records_of((dirs["cs"] / "g.block_alignments.paf").read_text())
    assert len(records) >= 6 and {r["sign"] for r in records} == {"+", "-"}
    kinds = set()
    for r in records:
        target, query = genomes[r["tg"]][r["t"]][r["t_from"]:r["t_to"]], genomes[r["qg"]][r["q"]][r["q_from"]:r["q_to"]]
        want = CS.reverse_complement(query) if r["sign"] == "-" else CS.letters(query)
        assert CS.apply_cs(r["cs"], target) == want, (r["tg"], r["qg"], r["t"], r["t_from"])
        assert CS.cigar_of_cs(r["cs"]) == r["cg"], (r["tg"], r["qg"], r["t"], r["t_from"])
        kinds |= {kind for kind, _ in CS.tokens(r["cs"])}
    assert kinds == set(":*-+")


def test_the_planted_deletion_of_40_bases(runs):
    """The deletion of 40 bases planted in genome 2 shows as `-` tokens that hold exactly 40 target bases, each token the target's own bases
    at its position, with no `+` among them.  The canonical script is a unit-cost one and takes a match wherever it can, so chance matches
    split the deletion into runs one or two `:` columns apart (tests/test_gpu_block_paf.py notes the same of the insertions): one `-` token
    of 40 bases is not what the aligner gives -- seen: 13 runs against genome 0, 8 against genome 1, 40 bases in both."""
    _, paths, dirs = runs
    genomes = {os.path.basename(p): {k: v.tobytes().decode() for k, v in read_fasta(p).items()} for p in paths}
    at, size, deleted = INDELS[0]
    assert (size, deleted) == (40, True)
    first = list(genomes["fam2.fa"])[0]                       # genome 2's first record holds the indels
    found = {}
    for r in records_of((dirs["cs"] / "g.block_alignments.paf").read_text()):
        if r["qg"] != "fam2.fa" or r["q"] != first:
            continue
        pos = r["t_from"]
        for kind, what in CS.tokens(r["cs"]):
            if abs(pos - at) < 100 and kind in "-+":
                assert kind == "-" and what == CS.letters(genomes[r["tg"]][r["t"]][pos:pos + len(what)]), (r["tg"], pos, kind, what)
                found[r["tg"]] = found.get(r["tg"], 0) + len(what)
            pos += what if kind == ":" else 1 if kind == "*" else len(what) if kind == "-" else 0
        assert pos == r["t_to"]
    print(found)
    assert found == {"fam0.fa": size, "fam1.fa": size}, found


def test_without_the_cs_column_the_file_is_that_of_block_paf_alone_and_every_other_file_is_equal(runs):
    _, _, dirs = runs
    with_cs = (dirs["cs"] / "g.block_alignments.paf").read_text()
    cut = "".join(line.rsplit("\t", 1)[0] + "\n" for line in with_cs.splitlines())
    assert all(line.rsplit("\t", 1)[1].startswith("cs:Z:") for line in with_cs.splitlines())
    assert cut.encode() == (dirs["plain"] / "g.block_alignments.paf").read_bytes()
    names = sorted(os.listdir(dirs["plain"]))
    assert names == sorted(os.listdir(dirs["cs"])) and "g.block_ends.tsv" in names
    for name in names:
        if name not in ("g.stage_times.tsv", "g.block_alignments.paf"):
            assert (dirs["plain"] / name).read_bytes() == (dirs["cs"] / name).read_bytes(), name
    stages = {name: [ln.split("\t")[0] for ln in (dirs[name] / "g.stage_times.tsv").read_text().splitlines()] for name in ("plain", "cs")}
    assert "block_paf:cigar_text_scan" in stages["cs"] and "block_paf:cigar_text_emit" in stages["cs"] and "block_paf:cigar_merge" in stages["cs"]
    assert [s for s in stages["cs"] if "cigar_text" not in s] == stages["plain"]


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, dirs = runs
    out, ends_out = tmp / "tool.block_alignments.paf", tmp / "tool.block_ends.tsv"
    fais = [str(dirs["cs"] / (os.path.basename(p) + ".fai")) for p in paths]
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["cs"] / "g.synteny_blocks.tsv"), "--fai"] + fais +
             ["--fastas"] + paths + ["--paf-out", str(out), "--paf-cs", "--identity-max-edits", "1023", "--ends-out", str(ends_out), "--ends-max-len", "1500",
                                     "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out.read_bytes() == (dirs["cs"] / "g.block_alignments.paf").read_bytes()
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["cs"] / "g.synteny_blocks.tsv"), "--fai"] + fais +
             ["--fastas"] + paths + ["--paf-cs"], tmp)
    assert r.returncode == 2 and "--paf-cs adds the cs:Z: tag to the records of --paf-out" in r.stderr, r.stderr[-500:]


def test_the_switch_needs_block_paf_and_one_rank(runs):
    tmp, paths, _ = runs
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    r = _run(ntsynt + paths + PARAMS + ["--paf-cs"], tmp)
    assert r.returncode == 2 and "--paf-cs adds the cs:Z: tag to the records of --block-paf" in r.stderr, r.stderr[-500:]
    r = _run(ntsynt + paths + PARAMS + ["--block-paf", "--paf-cs"], tmp, WORLD_SIZE="2")
    assert r.returncode == 2 and "ntsynt_block_stats" in r.stderr and "--paf-out <prefix>.block_alignments.paf --paf-cs" in r.stderr, r.stderr[-500:]
    r = _run(ntsynt + paths + PARAMS + ["--block-paf", "--paf-cs", "--dry-run"], tmp)
    assert r.returncode == 0 and "block_paf (cigar_atoms, cigar_merge, cigar_text_scan, cigar_text_emit; " in r.stdout + r.stderr, (r.stdout + r.stderr)[-800:]
