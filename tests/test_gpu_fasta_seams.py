"""The FASTA parse on the GPU (ntsynt_amd/csrc/nts_fasta_dev.inc: k_fa_scan, k_fa_headers / fa_find_nl, k_fa_bases<0/1>, k_fa_rec_off
and the host side of nts_genome_from_fasta) where a byte's place decides its path: headers, line ends and runs of blanks on the
seams of the 16 KiB tiles, of the 64-byte lanes and of the 4-byte words, files that end on a seam, lines that reach over whole
tiles, more headers than the first scan's table holds, every byte value beside a line feed, a blank and their one-bit twins, and
the 4096-byte limit of the blank walks.

The files are constructed (tests/fasta_cases.py; tests/test_fasta_cases_host.py checks on the CPU that every event stands where it
is claimed to, and that the plain parser there is the host reader).  Every expectation is parse(raw, blank_scan=4096), compared
exactly; outside the scan-limit group the native host reader must say the same (what tests/test_gpu_fasta.py: _same asserts).
Needs an MI355X."""
import faulthandler

import numpy as np
import pytest

from ntsynt_amd import fasta as fa
from tests import fasta_cases as FC

pytestmark = pytest.mark.gpu
STEP_SECONDS = 240
KS = (1, 20, 24)


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    from ntsynt_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def where(want, at):
    "base number `at` of the expected parse, as a place in the file"
    if at >= want.origin.size:
        return f"base {at}: behind the expected {want.origin.size}"
    off = int(want.origin[at])
    return f"base {at} = file offset {off} (offset % 16384 = {off % FC.TILE}, offset % 64 = {off % FC.LANE})"


def device_parse(ctx, path):
    "(records without bases, image, valid k-mers per k of KS) of one device parse"
    g, recs = fa.read_fasta_device(ctx, path)
    try:
        assert recs.seq is None and recs.names == g.names
        n = g.total_bp
        image = g.download(0, n) if n else np.zeros(0, np.uint8)
        return recs, n, image, [g.valid_kmers(k) for k in KS]
    finally:
        g.free()


def check_case(ctx, path, name, raw, scan_limit):
    from ntsynt_amd.device import Genome
    with open(path, "wb") as fh:
        fh.write(raw)
    want = FC.parse(raw, FC.BLANK_SCAN)
    recs, total, image, kmers = device_parse(ctx, path)
    assert recs.names == want.names, name
    lens, offs = recs.rec_len.tolist(), recs.rec_off.tolist()
    if lens != want.rec_len or offs != want.rec_off:
        r = next(i for i in range(len(lens)) if (lens[i], offs[i]) != (want.rec_len[i], want.rec_off[i]))
        raise AssertionError(f"{name}: record {r} ({want.names[r]!r}, header at file offset {want.hs[r]}, % 16384 = {want.hs[r] % FC.TILE}): "
                             f"offset, length {offs[r]}, {lens[r]}; expected {want.rec_off[r]}, {want.rec_len[r]}")
    expect = FC.codes(want.seq)
    if total != expect.size or not np.array_equal(image, expect):
        m = min(image.size, expect.size)
        diff = np.flatnonzero(image[:m] != expect[:m])
        at = int(diff[0]) if diff.size else m
        got = chr(image[at]) if at < image.size else "nothing"
        raise AssertionError(f"{name}: {total} bases, expected {expect.size}; first difference at {where(want, at)}: got {got}")
    assert recs.fai_rows == want.fai, (name, [(a, b) for a, b in zip(recs.fai_rows, want.fai) if a != b][:3])
    if expect.size:
        up = Genome(ctx, want.names, np.frombuffer(want.seq, dtype=np.uint8), np.array(want.rec_off, dtype=np.uint64),
                    np.array(want.rec_len, dtype=np.uint64))
        try:
            assert kmers == [up.valid_kmers(k) for k in KS], name
        finally:
            up.free()
    if not scan_limit:
        host = fa.read_fasta(path)
        assert recs.names == host.names and lens == host.rec_len.tolist() and offs == host.rec_off.tolist(), name
        assert recs.fai_rows == host.fai_rows and total == host.total_bp, name
        assert np.array_equal(image, FC.codes(host.seq)), name
    return want


@pytest.mark.parametrize("group", list(FC.GROUPS))
def test_device_parse_of_the_constructed_files(ctx, tmp_path, group):
    path = str(tmp_path / "case.fa")
    beyond = 0
    for name, raw, claims in FC.cases(group):
        want = check_case(ctx, path, name, raw, scan_limit=group == "scan_limit")
        if group == "scan_limit":                                 # the device keeps exactly the claimed number of blank bytes
            kept = len(want.seq) - len(FC.parse(raw).seq)
            assert kept == claims["scan_diff"], name
            beyond += kept
    assert (beyond > 0) == (group == "scan_limit")
    print(f"{group}: {len(FC.cases(group))} files")


def test_more_headers_than_the_first_table_holds(ctx, tmp_path):
    "1025, 3000 and 4097 records (a table of 1024: the scan runs twice), 1024 beside them: that many records, in file order"
    path = str(tmp_path / "count.fa")
    for n in FC.COUNT_RECORDS:
        name, raw, claims = FC.count_case(n)
        assert len(raw) < 65536
        with open(path, "wb") as fh:
            fh.write(raw)
        recs, total, image, _ = device_parse(ctx, path)
        assert len(recs.names) == n and recs.names == [f"r{i}" for i in range(n)], name
        assert recs.rec_len.tolist() == [4] * n and recs.rec_off.tolist() == list(range(0, 4 * n, 4)) and total == 4 * n, name
        assert bytes(image) == b"ACGT" * n, name
        assert recs.fai_rows[-1] == (f"r{n - 1}", 4, len(raw) - 5, 4, 5), name


def test_order_of_files_on_one_context(ctx, tmp_path):
    """the 4097-record file, the smallest case, the 4097-record file again on one context (fa_hdr, fa_tile_nl, fa_tile_cnt: grown,
    reused with stale content behind what a small file needs, grown again) == each on a fresh context"""
    from ntsynt_amd.device import Context
    big = FC.count_case(4097)
    small = min((c for g in FC.GROUPS for c in FC.cases(g)), key=lambda c: len(c[1]))
    paths = {}
    for name, raw, _ in (big, small):
        paths[name] = str(tmp_path / (name + ".fa"))
        with open(paths[name], "wb") as fh:
            fh.write(raw)

    def result(c, name):
        recs, total, image, kmers = device_parse(c, paths[name])
        return recs.names, recs.rec_off.tolist(), recs.rec_len.tolist(), recs.fai_rows, total, image.tobytes(), kmers

    fresh = {}
    for name in paths:
        c = Context(0)
        try:
            fresh[name] = result(c, name)
        finally:
            c.close()
    assert len(fresh[big[0]][0]) == 4097 and fresh[small[0]][4] == len(FC.parse(small[1], FC.BLANK_SCAN).seq)
    c = Context(0)
    try:
        for name in (big[0], small[0], big[0]):
            assert result(c, name) == fresh[name], name
    finally:
        c.close()
    for name in (big[0], small[0], big[0]):                       # and on the module's context, behind whatever ran before
        assert result(ctx, name) == fresh[name], name
