"""The constructed files of tests/fasta_cases.py hold what tests/test_gpu_fasta_seams.py relies on, and the plain parser there is the
host reader: every case's claims on its raw bytes, parse(raw) against the native reader (fa.read_fasta), against its numpy statement
(fa.read_fasta_numpy) and, where no sequence line holds white space inside (tests/test_gpu_fasta.py:
test_white_space_in_sequence_lines), against the oracle's reader; parse(raw, 4096), the device's rule, differs from it in the
scan-limit cases alone, by the claimed number of blank bytes.  No GPU."""
import numpy as np
import pytest

from ntsynt_amd import fasta as fa
from oracle import nts_oracle as O
from tests import fasta_cases as FC


def same_records(p, got, what):
    assert got.names == p.names, what
    assert got.rec_off.tolist() == p.rec_off and got.rec_len.tolist() == p.rec_len, what
    assert bytes(got.seq) == p.seq, what
    assert got.fai_rows == p.fai, what


@pytest.mark.parametrize("group", list(FC.GROUPS))
def test_cases_hold_their_claims_and_parse_is_the_host_reader(group, tmp_path):
    for name, raw, claims in FC.cases(group):
        p = FC.parse(raw)
        for what, fn in claims["facts"]:
            assert fn(raw, p), (name, what)
        assert p.origin.size == len(p.seq) == sum(p.rec_len) and [len(r) for r in p.records] == p.rec_len, name
        path = str(tmp_path / "case.fa")
        with open(path, "wb") as fh:
            fh.write(raw)
        same_records(p, fa.read_fasta(path), (name, "native reader"))
        same_records(p, fa.read_fasta_numpy(path), (name, "numpy statement"))
        if not p.interior:
            og = O.read_fasta(path)
            assert og.names == p.names and [og.record(i) for i in range(len(p.names))] == p.records, (name, "oracle")
        # the device's rule: the same parse but for the blank bytes beyond its scan limit, which stay as (invalid) bases
        d = FC.parse(raw, FC.BLANK_SCAN)
        extra = np.setdiff1d(d.origin, p.origin)
        assert extra.size == claims.get("scan_diff", 0) == len(d.seq) - len(p.seq), (name, extra.size)
        assert np.setdiff1d(p.origin, d.origin).size == 0 and all(raw[int(at)] in FC.BLANKS for at in extra), name
        assert (d.names, d.hs, d.he) == (p.names, p.hs, p.he), name
        if extra.size == 0:
            assert (d.seq, d.rec_off, d.rec_len, d.fai) == (p.seq, p.rec_off, p.rec_len, p.fai), name
        assert ("scan_diff" in claims) == (group == "scan_limit"), name


def test_the_groups_hold_the_cases_they_are_named_for():
    names = {g: [c[0] for c in FC.cases(g)] for g in FC.GROUPS}
    assert len({n for g in names.values() for n in g}) == sum(len(g) for g in names.values())
    for _, raw, _ in (c for g in FC.GROUPS for c in FC.cases(g)):
        assert len(raw) < 200 * 1024
    assert sum(len(c[1]) <= 5 * FC.TILE + 1024 for g in FC.GROUPS for c in FC.cases(g)) == sum(len(g) for g in names.values())
    # every case with LF and with CRLF line ends (the three empty records are longer with CRLF: more bytes to place)
    for g, ns in names.items():
        assert {n.replace("_crlf", "_lf") for n in ns if "_crlf" in n} >= {n for n in ns if "_crlf" not in n} != set(), g
    assert [c[2]["records"] for c in FC.cases("counts")] == list(FC.COUNT_RECORDS) * 2


def test_scan_limit_cases_differ_exactly_beyond_the_limit():
    "runs up to 4096 bytes and blank lines up to 8192 parse alike under both rules; one byte more is one invalid base more"
    seen = set()
    for name, raw, claims in FC.cases("scan_limit"):
        if "run" in claims:
            assert claims["scan_diff"] == max(0, claims["run"] - 4096), name
            seen.add(("run", claims["run"], claims["scan_diff"]))
        else:
            assert claims["scan_diff"] == max(0, claims["line"] - 8192), name
            seen.add(("line", claims["line"], claims["scan_diff"]))
        p, d = FC.parse(raw), FC.parse(raw, 4096)
        assert len(d.seq) - len(p.seq) == claims["scan_diff"], name
        kind = "trailing" if "trailing" in name else "leading" if "leading" in name else "line"
        extra = np.setdiff1d(d.origin, p.origin)
        if extra.size:                                            # which bytes stay: the far end of a run, the middle of a line
            run = next(at for at in range(int(extra[0]), -1, -1) if raw[at - 1] not in FC.BLANK_CLASS)
            n = claims.get("run", claims.get("line"))
            lo = {"trailing": run, "leading": run + 4096, "line": run + 4096}[kind]
            assert extra.tolist() == list(range(lo, lo + claims["scan_diff"])), (name, run, extra[:3])
            assert FC.codes(bytes(raw[int(at)] for at in extra)).tolist() == [ord("N")] * extra.size
            assert n > 4096
    assert seen == {("run", 4095, 0), ("run", 4096, 0), ("run", 4097, 1), ("line", 8191, 0), ("line", 8192, 0), ("line", 8193, 1),
                    ("line", 10000, 1808)}


def test_the_expected_image_is_the_mapping_of_the_existing_module():
    from tests.test_gpu_fasta import _codes
    every = bytes(range(256))
    assert np.array_equal(FC.codes(every), _codes(every))
    assert bytes(FC.codes(b"ACGTUacgtuNn \t>\x00\xc1")) == b"ACGTTACGTTNNNNNNN"


def test_parse_on_the_small_files_of_the_existing_module(tmp_path):
    "the rules in words give the records that tests/test_gpu_fasta.py spells out"
    raw = (b">a desc\nACGT  \nAC\t\n \tGGT\r\nTT AC\n\x0c\n>b\n   \nACGTACGT \t \r\nAC\tGT\n>c\nAAAA   ")
    p = FC.parse(raw)
    assert p.names == ["a", "b", "c"] and p.records == [b"ACGTACGGTTT AC", b"ACGTACGTAC\tGT", b"AAAA"] and p.interior
    assert p.fai[0][3:] == (4, 7) and p.fai[2][3:] == (4, 7)
    for raw in (b"", b"\n \n", b">only\n", b">a\nAC\n\nGT\n>b x y\n", b"junk\n>a\tdesc\r\nAC\r\nG\r\n>b\r\n\r\nT", b">a\nACGT",
                b">a\n>b\n>c\nACGTNNacgtnRYKM\n", b">x y z\nACGU\nacgu", b">a\n\nACGT\n", b">a\n\r\nACGT\n", b">a\n  \nACGT\n"):
        path = str(tmp_path / "small.fa")
        with open(path, "wb") as fh:
            fh.write(raw)
        same_records(FC.parse(raw), fa.read_fasta(path), raw)
        same_records(FC.parse(raw), fa.read_fasta_numpy(path), raw)
