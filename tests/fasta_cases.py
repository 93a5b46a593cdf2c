"""FASTA files whose events are CONSTRUCTED onto the seams of the GPU parse (tests/test_gpu_fasta_seams.py; checked on the CPU by
tests/test_fasta_cases_host.py), and a plain statement of the parsing rules.  Plain Python and numpy; never the library under test.

The parse (ntsynt_amd/csrc/nts_fasta_dev.inc) cuts the file into tiles of TILE = 16384 bytes, a lane takes LANE = 64 of them as
sixteen 4-byte words.  A whole tile is PLAIN when a header lies before it whose line ended before the tile and no header starts
inside it (plain_tiles); the kernels take such a tile through registers and every other byte one by one.

The rules, as parse() states them line by line:
  * a header is '>' at offset 0 or right after a line feed; the record id is its text up to the first blank, tab, CR, VT or FF;
  * nothing before the first header is sequence;
  * in a sequence line carriage returns go wherever they are; blanks, tabs, VT and FF go where they run up to the line's start or
    to its end (the line feed, or the end of the file); every other byte stays, white space inside a line included;
  * the faidx columns bases-per-line and bytes-per-line are those of the first line after the header (the bytes with the line's
    terminator); both are 0 when that line is empty, is the next header, or the record has no bases.
blank_scan=None is the host reader's rule: runs of any length are trimmed.  blank_scan=4096 is the device's: a blank byte goes
only if FEWER than 4096 blank bytes (carriage returns count: the device walks over them) lie between it and the line's start, or
between it and the line's end -- a leading run of a bytes keeps its last max(0, a - 4096), a trailing run of b its first
max(0, b - 4096), a line of L blank bytes max(0, L - 8192), as invalid bases.

A case is (name, raw, claims): claims["facts"] is a list of (what, fn(raw, parsed)) that the host test asserts, so that an edit to
a constructor cannot move an event off its seam unnoticed; claims["scan_diff"] (0 when absent) is the number of blank bytes that
parse(raw, 4096) keeps and parse(raw) drops."""
import zlib

import numpy as np

TILE, LANE = 16384, 64
BLANK_SCAN = 4096
LF, CR, GT = 10, 13, ord(">")
BLANKS = b" \t\v\f"
BLANK_CLASS = BLANKS + b"\r"                                     # what the trimming walks over
EOLS = (("lf", b"\n"), ("crlf", b"\r\n"))


# ---- the rules ---------------------------------------------------------------------------------------------------------------------------
class Parsed:
    """names, records (bytes per record), fai (name, length, offset, linebases, linewidth), seq / rec_off / rec_len as the readers
    give them, hs / he (offsets of every header's '>' and of its line feed, the file size where it has none), keep (per byte of the
    file: is a base), origin (file offset of every base), interior (a sequence line holds white space or a CR inside)"""


def codes(seq):
    "what the resident genome reads back as: A/C/G/T (U -> T) upper case, anything else N (tests/test_gpu_fasta.py: _codes)"
    a = np.frombuffer(bytes(seq), dtype=np.uint8).copy() & 0xDF
    out = np.full(a.size, ord("N"), np.uint8)
    for c in b"ACGT":
        out[a == c] = c
    out[a == ord("U")] = ord("T")
    return out


def parse(raw, blank_scan=None):
    raw = bytes(raw)
    n = len(raw)
    keep = bytearray(n)
    names, fai, hs, he = [], [], [], []
    interior = False
    in_record = first_line = False
    i = 0
    while i < n:
        e = raw.find(b"\n", i)
        has_nl = e >= 0
        if not has_nl:
            e = n
        line = raw[i:e]
        if line[:1] == b">":
            j = 1
            while j < len(line) and line[j] not in BLANK_CLASS:
                j += 1
            names.append(line[1:j].decode())
            hs.append(i)
            he.append(e)
            fai.append([e + 1 if has_nl else n, 0, 0])
            in_record = first_line = True
        elif in_record:
            L = len(line)
            a = L - len(line.lstrip(BLANK_CLASS))                 # the run at the line's start
            b = L - len(line.rstrip(BLANK_CLASS))                 # the run at its end (the whole line, if it is all blank)
            kept = 0
            if blank_scan is None or (a <= blank_scan and b <= blank_scan):
                if a < L:                                         # both runs go whole; of what is between them, the CRs
                    keep[i + a:i + L - b] = b"\x01" * (L - b - a)
                    kept = L - b - a
                    j = line.find(b"\r", a, L - b)
                    while j >= 0:
                        keep[i + j] = 0
                        kept -= 1
                        j = line.find(b"\r", j + 1, L - b)
            else:
                for j in range(L):
                    c = line[j]
                    if c == CR:
                        continue
                    if c in BLANKS and ((j < a and j < blank_scan) or (j >= L - b and L - 1 - j < blank_scan)):
                        continue
                    keep[i + j] = 1
                    kept += 1
            core = line[a:L - b] if a < L else b""
            if any(c in core for c in BLANK_CLASS):
                interior = True
            if first_line:
                if L > 0:
                    fai[-1][1:] = [kept, L + (1 if has_nl else 0)]
                first_line = False
        i = e + 1 if has_nl else n
    p = Parsed()
    p.keep = keep
    p.origin = np.flatnonzero(np.frombuffer(bytes(keep), dtype=np.uint8)).astype(np.int64)
    p.seq = bytes(np.frombuffer(raw, dtype=np.uint8)[p.origin]) if n else b""
    bases_before = np.concatenate(([0], np.cumsum(np.frombuffer(bytes(keep), dtype=np.uint8), dtype=np.int64)))
    stops = hs[1:] + [n]
    p.names, p.hs, p.he, p.interior = names, hs, he, interior
    p.rec_off = [int(bases_before[s]) for s in hs]
    p.rec_len = [int(bases_before[t] - bases_before[s]) for s, t in zip(hs, stops)]
    p.records = [p.seq[o:o + ln] for o, ln in zip(p.rec_off, p.rec_len)]
    p.fai = [(nm, ln, off, lb if ln else 0, lw if ln else 0) for nm, ln, (off, lb, lw) in zip(names, p.rec_len, fai)]
    return p


def plain_tiles(raw, p):
    "per whole tile of the file: is it plain (see the module's docstring)"
    out = []
    for t in range(len(raw) // TILE):
        lo = t * TILE
        r = int(np.searchsorted(np.array(p.hs, dtype=np.int64), lo, side="right")) - 1
        out.append(r >= 0 and p.he[r] < lo and (r + 1 >= len(p.hs) or p.hs[r + 1] >= lo + TILE))
    return out


# ---- facts -------------------------------------------------------------------------------------------------------------------------------
def byte_at(off, c):
    c = c if isinstance(c, int) else c[0]
    return (f"byte {c:#04x} at {off}", lambda raw, p: raw[off] == c)


def header_at(off):
    return (f"a header starts at {off}", lambda raw, p: raw[off] == GT and off in p.hs)


def not_header(off):
    return (f"the '>' at {off} is a base", lambda raw, p: raw[off] == GT and off not in p.hs and p.keep[off] == 1)


def header_lf_at(off):
    return (f"a header line ends at {off}", lambda raw, p: off in p.he and (off == len(raw) or raw[off] == LF))


def is_plain(t, what=True):
    return (f"tile {t} plain: {what}", lambda raw, p: plain_tiles(raw, p)[t] == what)


def kept(lo, hi=None):
    hi = lo + 1 if hi is None else hi
    return (f"bytes {lo}..{hi - 1} are bases", lambda raw, p: hi > lo and all(p.keep[lo:hi]))


def dropped(lo, hi=None):
    hi = lo + 1 if hi is None else hi
    return (f"bytes {lo}..{hi - 1} are dropped", lambda raw, p: hi > lo and not any(p.keep[lo:hi]))


def blank_bytes(lo, hi):
    return (f"bytes {lo}..{hi - 1} are blanks", lambda raw, p: hi > lo and all(c in BLANKS for c in raw[lo:hi]))


def size_is(n):
    return (f"the file has {n} bytes", lambda raw, p: len(raw) == n)


def records_are(n):
    return (f"{n} records", lambda raw, p: len(p.names) == n)


def no_lf_in_tile(t):
    return (f"tile {t} holds no line feed", lambda raw, p: len(raw) >= (t + 1) * TILE and LF not in raw[t * TILE:(t + 1) * TILE])


# ---- building ----------------------------------------------------------------------------------------------------------------------------
ALPHABET = np.frombuffer(b"ACGTACGTACGTNacgtn", dtype=np.uint8)
TEXT = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 \t>_=|;,.", dtype=np.uint8)


class Build:
    "a file written front to back: a first header (unless first=None), then whatever is added; filler lines of 60 and 61 bases"

    def __init__(self, name, eol=b"\n", first=b">r0 first record\tof the file"):
        self.name, self.eol = name, eol
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.buf = bytearray()
        self.lines = 0
        self.facts = []
        if first is not None:
            self.add(first + eol)

    @property
    def pos(self):
        return len(self.buf)

    def add(self, data):
        at = len(self.buf)
        self.buf += data
        return at

    def bases(self, n):
        return ALPHABET[self.rng.integers(0, ALPHABET.size, size=int(n))].tobytes()

    def text(self, n):
        "header text: letters, digits, blanks, tabs, '>' -- no line end"
        return TEXT[self.rng.integers(0, TEXT.size, size=int(n))].tobytes()

    def _line(self, width, junk):
        if junk:                                                  # what may stand before the first header: no '>' or '@' at its start
            return b"j" + self.text(width - 1)
        return self.bases(width)

    def fill(self, target, open_line=False, junk=False):
        """filler lines up to exactly `target`.  The last line ends at target - 1 with its terminator, or (open_line) is left
        without one for the caller to go on with: at least one base, unless nothing was to be filled"""
        e = len(self.eol)
        assert target >= self.pos, (self.name, target, self.pos)
        while True:
            room = target - self.pos
            if room == 0:
                return
            w = 60 + (self.lines & 1)
            self.lines += 1
            if room >= w + e + 1 + e:
                self.add(self._line(w, junk) + self.eol)
            elif open_line:
                if room > w + e:
                    self.add(self._line(w, junk) + self.eol)
                    continue
                self.add(self._line(room, junk))
                return
            else:
                assert room >= 1 + e, (self.name, target, room)
                self.add(self._line(room - e, junk) + self.eol)
                return

    def header_ending_at(self, at, stem):
        "fill, then a header line whose line feed stands at `at`; returns where its '>' stands"
        line = b">" + stem + self.eol
        self.fill(at + 1 - len(line))
        start = self.add(line)
        assert self.pos == at + 1
        return start

    def tail(self, whole=1, extra=777):
        "filler over `whole` more whole tiles and a partial last one"
        self.fill((self.pos // TILE + 1 + whole) * TILE + extra)

    def case(self, **claims):
        claims["facts"] = self.facts
        return (self.name, bytes(self.buf), claims)


def blanks(n, mixed):
    "n blank bytes: blanks and tabs, or (mixed) vertical tabs and form feeds among them"
    unit = b" \t\v \f\t" if mixed else b" \t"
    return (unit * (n // len(unit) + 1))[:n]


# ---- headers at seams --------------------------------------------------------------------------------------------------------------------
def header_cases():
    out = []
    for en, eol in EOLS:
        for t in (1, 2):
            S = t * TILE
            for d in (0, 1, 2, 20):                               # '>' at S - d: at the tile's first byte, or its line crosses
                b = Build(f"hdr_gt_at_S-{d}_{en}_t{t}", eol)
                b.fill(S - d)
                at = b.add(b">seam%d a header line that is long enough to cross the seam" % d + eol)
                b.tail()
                b.facts += [header_at(S - d), byte_at(S - d - 1, LF), is_plain(t, False),
                            (f"its line ends behind {S}", lambda raw, p, at=at, S=S: p.he[p.hs.index(at)] > S)]
                out.append(b.case())
            for x in (-1, 0, 1):                                  # a header's line feed at S - 1 (the tile behind is plain), S, S + 1
                b = Build(f"hdr_lf_at_S{x:+d}_{en}_t{t}", eol)
                b.header_ending_at(S + x, b"lf_here and some description")
                b.tail()
                b.facts += [header_lf_at(S + x), is_plain(t, x == -1)]
                out.append(b.case())
            for d in (0, 1):                                      # the next header at S + TILE (tile t plain) and one byte before
                b = Build(f"next_hdr_at_S+{TILE - d}_{en}_t{t}", eol)
                b.fill(S + TILE - d)
                b.add(b">next header" + eol)
                b.tail(whole=0)
                b.facts += [header_at(S + TILE - d), is_plain(t, d == 0), byte_at(S + TILE - d - 1, LF)]
                out.append(b.case())
            block = b">a" + eol + b">b" + eol + b">c" + eol       # three empty records, every byte of theirs at S in turn
            for j in range(len(block)):
                b = Build(f"empty_records_byte{j}_at_S_{en}_t{t}", eol)
                b.fill(S - j)
                b.add(block)
                b.tail()
                starts = [S - j, S - j + 2 + len(eol), S - j + 4 + 2 * len(eol)]
                b.facts += [byte_at(S, block[j]), records_are(4)] + [header_at(s) for s in starts]
                b.facts.append(("records a and b are empty", lambda raw, p: p.names[1:] == ["a", "b", "c"] and p.rec_len[1:3] == [0, 0]
                                and p.rec_len[3] > TILE))
                out.append(b.case())
    return out


def lane_cases():
    """'>' at the first byte of every lane of tile 1 and once more inside every lane, at all four word offsets: behind a line feed
    (headers: 513 records), and behind an A, a lone CR, a blank, a tab (no header: the byte is a base, the tile is plain)"""
    out = []
    S = TILE
    stamps = sorted([S + LANE * ln for ln in range(256)] + [S + LANE * ln + 32 + ln % 4 for ln in range(256)])
    for en, eol in EOLS:
        for pn, prev in (("lf", eol), ("A", b"A"), ("cr", b"\r"), ("blank", b" "), ("tab", b"\t")):
            b = Build(f"lanes_gt_behind_{pn}_{en}", eol)
            b.fill(S - LANE)
            start = b.pos
            block = bytearray(b.bases(LANE + TILE + LANE))
            for at in stamps:
                i = at - start
                block[i] = GT
                block[i - len(prev):i] = prev
                if pn == "lf":
                    block[i + 1:i + 2 + len(eol)] = b"h" + eol
                else:
                    block[i + 12:i + 12 + len(eol)] = eol
            b.add(bytes(block) + eol)
            b.tail()
            b.facts.append(("every lane's first byte and all four word offsets",
                            lambda raw, p: {s % TILE for s in stamps} >= set(range(0, TILE, LANE)) and {s % 4 for s in stamps} == {0, 1, 2, 3}))
            if pn == "lf":
                b.facts += [header_at(s) for s in stamps] + [byte_at(s - 1, LF) for s in stamps] + [records_are(1 + len(stamps))]
            else:
                b.facts += [not_header(s) for s in stamps] + [byte_at(s - 1, prev) for s in stamps] + [records_are(1), is_plain(1)]
                b.facts += [dropped(s - 1) if pn == "cr" else kept(s - 1) for s in stamps]
            out.append(b.case())
    return out


# ---- line ends at seams ------------------------------------------------------------------------------------------------------------------
def line_end_cases():
    out = []
    for en, eol in EOLS:
        for t in (1, 2):
            S = t * TILE
            b = Build(f"cr_at_S-1_lf_at_S_{en}_t{t}", eol)
            b.fill(S - 1, open_line=True)
            b.add(b"\r\n")
            b.tail()
            b.facts += [byte_at(S - 1, CR), byte_at(S, LF), kept(S - 2)]
            out.append(b.case())
            for x in (-1, 0):
                b = Build(f"lf_at_S{x:+d}_{en}_t{t}", eol)
                b.fill(S + x + 1)
                b.tail()
                b.facts += [byte_at(S + x, LF), kept(S + x + 1)]
                out.append(b.case())
            b = Build(f"empty_line_at_S_{en}_t{t}", eol)
            b.fill(S)
            b.add(eol)
            b.tail()
            b.facts += [byte_at(S - 1, LF), byte_at(S + len(eol) - 1, LF), dropped(S, S + len(eol))]
            out.append(b.case())
            b = Build(f"empty_first_line_at_S_{en}_t{t}", eol)
            b.header_ending_at(S - 1, b"empty_first line")
            b.add(eol)
            b.tail()
            b.facts += [header_lf_at(S - 1), byte_at(S + len(eol) - 1, LF),
                        ("the record has bases, its first line none", lambda raw, p, eol=eol: p.fai[1][1] > 0 and
                         p.fai[1][3:] == ((0, 0) if eol == b"\n" else (0, 2)))]
            out.append(b.case())
        for tiles in (1, 2, 3):                                   # tiles without any line feed: a single-line record over them
            S = TILE
            b = Build(f"single_line_over_{tiles}_tiles_{en}", eol)
            b.header_ending_at(S - 5, b"single line")
            b.add(b.bases(4 + tiles * TILE + 4) + eol)
            after = b.add(b">after" + eol)
            b.tail(whole=0)
            b.facts += [no_lf_in_tile(1 + j) for j in range(tiles)] + [header_at(after), is_plain(1),
                        ("the first line's columns", lambda raw, p, w=8 + tiles * TILE, eol=eol: p.fai[1][3:] == (w, w + len(eol)))]
            out.append(b.case())
        b = Build(f"last_record_without_lf_{en}", eol)
        b.fill(TILE + 100)
        at = b.add(b">last" + eol)
        b.add(b.bases(2 * TILE))
        b.facts += [header_at(at), ("no line feed behind the last header line", lambda raw, p, at=at: raw.count(b"\n", at) == 1),
                    ("the file ends in a base", lambda raw, p: p.keep[len(raw) - 1] == 1)]
        out.append(b.case())
    return out


# ---- blanks at seams ---------------------------------------------------------------------------------------------------------------------
def _run_places(S, n):
    "where a run of n blanks ends: its last byte at S - 1, at S, or the run across S"
    places = [("ends_at_S-1", S - 1), ("ends_at_S", S)]
    if n >= 2:
        places.append(("crosses_S", S - 1 + n // 2))
    return places


def blank_cases():
    out = []

    def done(b, sn):
        if sn == "lane100":
            b.facts.append(is_plain(2))
        out.append(b.case())

    for en, eol in EOLS:
        for S, sn in ((TILE, "t1"), (2 * TILE, "t2"), (2 * TILE + 100 * LANE, "lane100")):      # the last: a lane boundary in a plain tile
            for n in (1, 2, 5, 70):
                if sn == "lane100" and n == 1:
                    continue
                run = blanks(n, mixed=n >= 5)
                for pn, last in _run_places(S, n):
                    if sn == "lane100" and pn != "crosses_S":
                        continue
                    first = last - n + 1
                    b = Build(f"trailing_{n}_{pn}_{en}_{sn}", eol)
                    b.fill(first, open_line=True)
                    b.add(run + eol)
                    b.tail()
                    b.facts += [blank_bytes(first, last + 1), dropped(first, last + 1), kept(first - 1), byte_at(last + len(eol), LF)]
                    done(b, sn)
                    b = Build(f"leading_{n}_{pn}_{en}_{sn}", eol)
                    b.fill(first)
                    b.add(run + b.bases(30) + eol)
                    b.tail()
                    b.facts += [blank_bytes(first, last + 1), dropped(first, last + 1), kept(last + 1), byte_at(first - 1, LF)]
                    done(b, sn)
                if n >= 2:
                    last = S - 1 + n // 2
                    first = last - n + 1
                    b = Build(f"interior_{n}_crosses_S_{en}_{sn}", eol)                        # a base before, a base behind: it stays
                    b.fill(first, open_line=True)
                    b.add(run + b.bases(20) + eol)
                    b.tail()
                    b.facts += [blank_bytes(first, last + 1), kept(first - 1, last + 2)]
                    done(b, sn)
                    b = Build(f"blank_line_{n}_crosses_S_{en}_{sn}", eol)
                    b.fill(first)
                    b.add(run + eol)
                    b.tail()
                    b.facts += [blank_bytes(first, last + 1), dropped(first, last + 1 + len(eol)), byte_at(first - 1, LF)]
                    done(b, sn)
    return out


# ---- the scan limit ----------------------------------------------------------------------------------------------------------------------
def scan_limit_cases():
    """runs of 4095, 4096, 4097 blank bytes at a line's end and at its start, inside tile 2 and across the seam before it, and lines
    of 8191, 8192, 8193, 10000 blank bytes: the lengths count the CR of a CRLF line end, which the device walks over like a blank"""
    out = []
    S = 2 * TILE
    for en, eol in EOLS:
        cr = len(eol) - 1
        for where, first in (("inside", S + 5000), ("crossing", S - 2000)):
            for n in (BLANK_SCAN - 1, BLANK_SCAN, BLANK_SCAN + 1):
                over = max(0, n - BLANK_SCAN)
                b = Build(f"scan_trailing_{n}_{where}_{en}", eol)
                b.fill(first, open_line=True)
                b.add(blanks(n - cr, mixed=True) + eol)
                b.tail()
                b.facts += [blank_bytes(first, first + n - cr), byte_at(first + n, LF), kept(first - 1), dropped(first, first + n)]
                if where == "inside":
                    b.facts.append(("the run lies in one plain tile", lambda raw, p, lo=first, hi=first + n: lo // TILE == hi // TILE == 2
                                    and plain_tiles(raw, p)[2]))
                else:
                    b.facts.append(("the run crosses the seam", lambda raw, p, lo=first, hi=first + n: lo < S < hi))
                out.append(b.case(scan_diff=over, run=n))
                b = Build(f"scan_leading_{n}_{where}_{en}", eol)
                b.fill(first)
                b.add(blanks(n, mixed=True) + b.bases(40) + eol)
                b.tail()
                b.facts += [blank_bytes(first, first + n), byte_at(first - 1, LF), kept(first + n), dropped(first, first + n)]
                out.append(b.case(scan_diff=over, run=n))
        for n in (2 * BLANK_SCAN - 1, 2 * BLANK_SCAN, 2 * BLANK_SCAN + 1, 10000):
            first = S + 10000
            b = Build(f"scan_blank_line_{n}_{en}", eol)
            b.fill(first)
            b.add(blanks(n - cr, mixed=True) + eol)
            b.tail()
            b.facts += [blank_bytes(first, first + n - cr), byte_at(first - 1, LF), byte_at(first + n, LF), dropped(first, first + n),
                        ("the line crosses a seam", lambda raw, p, lo=first, hi=first + n: lo < 3 * TILE < hi)]
            out.append(b.case(scan_diff=max(0, n - 2 * BLANK_SCAN), line=n))
    return out


# ---- file ends ---------------------------------------------------------------------------------------------------------------------------
def file_end_cases():
    out = []
    for en, eol in EOLS:
        for t in (1, 3):
            N = t * TILE
            b = Build(f"size_{t}_tiles_ends_in_base_{en}", eol)
            b.fill(N, open_line=True)
            b.facts += [size_is(N), kept(N - 1)]
            out.append(b.case())
            b = Build(f"size_{t}_tiles_ends_in_lf_{en}", eol)
            b.fill(N)
            b.facts += [size_is(N), byte_at(N - 1, LF)]
            out.append(b.case())
            b = Build(f"size_{t}_tiles_ends_in_cr_{en}", eol)
            b.fill(N - 1, open_line=True)
            b.add(b"\r")
            b.facts += [size_is(N), byte_at(N - 1, CR), kept(N - 2)]
            out.append(b.case())
            tail = b">tail header without a line end"
            b = Build(f"size_{t}_tiles_ends_in_header_{en}", eol)
            b.fill(N - len(tail))
            b.add(tail)
            b.facts += [size_is(N), header_at(N - len(tail)), header_lf_at(N)]
            out.append(b.case())
            b = Build(f"size_{t}_tiles_ends_in_blanks_{en}", eol)
            b.fill(N - 5, open_line=True)
            b.add(b" \t \x0c\t")
            b.facts += [size_is(N), dropped(N - 5, N), kept(N - 6)]
            out.append(b.case())
            for x in (-1, 1):                                     # (+1: a last tile of one byte)
                b = Build(f"size_{t}_tiles{x:+d}_ends_in_base_{en}", eol)
                b.fill(N + x, open_line=True)
                b.facts += [size_is(N + x), kept(N + x - 1)]
                out.append(b.case())
                b = Build(f"size_{t}_tiles{x:+d}_ends_in_lf_{en}", eol)
                b.fill(N + x)
                b.facts += [size_is(N + x), byte_at(N + x - 1, LF)]
                out.append(b.case())
            b = Build(f"size_{t}_tiles+1_ends_in_gt_{en}", eol)    # the one byte is a header: a record without id, without bases
            b.fill(N)
            b.add(b">")
            b.facts += [size_is(N + 1), header_at(N), ("the last record has no id", lambda raw, p: p.names[-1] == "" and p.rec_len[-1] == 0)]
            out.append(b.case())
    return out


# ---- long lines: the per-tile table of first line feeds ----------------------------------------------------------------------------------
def long_line_cases():
    out = []
    for en, eol in EOLS:
        b = Build(f"header_of_20000_bytes_{en}", eol)
        b.fill(5000)
        at = b.add(b">long ")
        b.add(b.text(20000 - 6 - len(eol)) + eol)
        b.tail()
        b.facts += [header_at(at), header_lf_at(at + 19999), ("the line ends in the next tile", lambda raw, p, at=at: (at + 19999) // TILE == at // TILE + 1)]
        out.append(b.case())
        b = Build(f"header_lf_first_byte_two_tiles_on_{en}", eol)
        b.fill(TILE + 300)
        at = b.add(b">far ")
        b.add(b.text(3 * TILE - b.pos - len(eol) + 1) + eol)
        b.tail()
        b.facts += [header_at(TILE + 300), header_lf_at(3 * TILE), no_lf_in_tile(2), is_plain(3, False)]
        out.append(b.case())
        b = Build(f"first_line_ends_three_tiles_on_{en}", eol)
        b.fill(TILE + 100)
        at = b.add(b">wide" + eol)
        b.add(b.bases(3 * TILE) + eol)
        b.tail(whole=0)
        b.facts += [header_at(at), no_lf_in_tile(2), no_lf_in_tile(3),
                    ("the first line ends three tiles on", lambda raw, p, at=at: raw.find(b"\n", p.he[p.hs.index(at)] + 1) // TILE == at // TILE + 3)]
        out.append(b.case())
        b = Build(f"header_without_lf_last_18000_bytes_{en}", eol)
        b.fill(TILE + 500)
        at = b.add(b">nolf ")
        b.add(b.text(18000 - 6))
        b.facts += [header_at(at), header_lf_at(b.pos), ("the last 18000 bytes", lambda raw, p, at=at: len(raw) - at == 18000 and LF not in raw[at:])]
        out.append(b.case())
    return out


# ---- before the first header -------------------------------------------------------------------------------------------------------------
def junk_cases():
    out = []
    for en, eol in EOLS:
        for at, what in ((20011, "unaligned"), (2 * TILE, "at_S")):
            b = Build(f"junk_before_first_header_{what}_{en}", eol, first=None)
            b.fill(at, junk=True)
            b.add(b">first header behind the junk" + eol)
            b.tail(whole=0)
            b.facts += [header_at(at), ("it is the first header, more than a tile in", lambda raw, p, at=at: p.hs[0] == at > TILE),
                        ("the junk holds '>' and blanks", lambda raw, p, at=at: raw.count(b">", 0, at) > 50 and raw.count(b" ", 0, at) > 50),
                        dropped(0, at)]
            out.append(b.case())
    return out


# ---- more headers than the first attempt's table holds -----------------------------------------------------------------------------------
COUNT_RECORDS = (1024, 1025, 3000, 4097)


def count_case(n, en="lf"):
    eol = dict(EOLS)[en]
    b = Build(f"records_{n}_{en}", eol, first=None)
    b.add(b"".join(b">r%d" % i + eol + b"ACGT" + eol for i in range(n)))
    b.facts += [records_are(n), ("under 64 KiB: a table of 1024 headers at first", lambda raw, p: len(raw) < 65536 and max(1024, len(raw) // 4096) == 1024),
                ("in file order", lambda raw, p: p.names == [f"r{i}" for i in range(n)] and p.records == [b"ACGT"] * n)]
    return b.case(records=n)


def count_cases():
    return [count_case(n, en) for en, _ in EOLS for n in COUNT_RECORDS]


# ---- byte values -------------------------------------------------------------------------------------------------------------------------
TWINS = (0x8A, 0x0B, 0xBE, 0x3F)                                  # one bit away from the line feed (0x0A) and from '>' (0x3E)


def byte_value_cases():
    """every byte value but LF and '>' at each of the four positions of a word, beside a line feed, a blank, and each of the four
    twins in the same word (the neighbour behind it in one file, before it in the other), all inside whole plain tiles"""
    out = []
    values = [v for v in range(256) if v not in (LF, GT)]
    for en, eol in EOLS:
        for side, step in (("behind", 1), ("before", 3)):
            b = Build(f"byte_values_neighbour_{side}_{en}", eol)
            b.fill(TILE)
            lo = b.pos
            for v in values:
                for at in range(4):
                    for nb in (LF, ord(" ")) + TWINS:
                        word = bytearray(b"ACGT")
                        word[at] = v
                        word[(at + step) % 4] = nb
                        b.add(bytes(word) + b"acgt")
            hi = b.pos
            b.add(eol)
            b.fill(4 * TILE + 500)
            b.facts += [("the words lie in tiles 1 to 3, word-aligned", lambda raw, p, lo=lo, hi=hi: lo == TILE and lo % 4 == 0 and hi <= 4 * TILE
                         and hi - lo == 254 * 4 * 6 * 8), is_plain(1), is_plain(2), is_plain(3), records_are(1)]
            out.append(b.case())
    return out


GROUPS = {"headers": header_cases, "lanes": lane_cases, "line_ends": line_end_cases, "blanks": blank_cases, "scan_limit": scan_limit_cases,
          "file_ends": file_end_cases, "long_lines": long_line_cases, "junk": junk_cases, "counts": count_cases, "byte_values": byte_value_cases}
_built = {}


def cases(group):
    "the cases of a group, built once and left unchanged"
    if group not in _built:
        _built[group] = GROUPS[group]()
        names = [c[0] for c in _built[group]]
        assert len(set(names)) == len(names), group
    return _built[group]
