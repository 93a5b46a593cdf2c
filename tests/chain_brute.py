"""Brute force for nts_cigar_chain_blocks and the chain file (docs/design/04_28_block_chain.md), the definition taken literally, in pure
Python without a device: brute_blocks walks each pair's linked chains in link order as a list of match runs and gaps and collects the
blocks; brute_text renders them; parse_chain is a strict reader of the UCSC chain format; lift_base is liftOver's per-base rule;
chains_from_paf builds the expected file from a run's PAF text alone."""
from tests import lift_brute as LB

I, D, EQ, X = 1, 2, 7, 8


def pair_items(cigar, chains, links, l0, l1):
    """the pair's columns in link order as items: ("m", code, n, a, b) -- n match columns of one kind that start at (a, b) in the pair's
    oriented offsets -- and ("g", da, db) -- a gap: a D entry, an I entry or the open stretch in front of a link"""
    items, end = [], None
    for i in range(l0, l1):
        c, a, b = int(links[i]["chain"]), int(links[i]["a0"]), int(links[i]["b0"])
        if end is not None:
            assert a >= end[0] and b >= end[1]
            items.append(("g", a - end[0], b - end[1]))
        first, n = int(chains[c]["first"]), int(chains[c]["n_cig"])
        for v in (int(v) for v in cigar[first:first + n]):
            code, length = v & 15, v >> 4
            assert code in (I, D, EQ, X) and length > 0
            if code in (EQ, X):
                items.append(("m", code, length, a, b))
                a, b = a + length, b + length
            elif code == D:
                items.append(("g", length, 0))
                a += length
            else:
                items.append(("g", 0, length))
                b += length
        assert (a, b) == (int(links[i]["a0"]) + int(chains[c]["len_a"]), int(links[i]["b0"]) + int(chains[c]["len_b"]))
        end = (a, b)
    return items


def brute_blocks(cigar, chains, links, pair_first):
    """(pairs, blocks): pairs[p] = (a0, a1, b0, b1, eq, x, first_block, n_blocks), all 0 for a pair without a match column; blocks =
    [(size, dt, dq)] of all pairs one behind the other"""
    pairs, blocks = [], []
    for p in range(len(pair_first) - 1):
        mine, gap, eq, x, span = [], (0, 0), 0, 0, None
        for item in pair_items(cigar, chains, links, int(pair_first[p]), int(pair_first[p + 1])):
            if item[0] == "g":
                gap = (gap[0] + item[1], gap[1] + item[2])
                continue
            _, code, n, a, b = item
            if not mine:                                      # the pair's first match column: the gaps in front of it belong to no block
                mine.append([0, 0, 0])
                span = [a, a, b, b]
            elif gap != (0, 0):                               # a gap of non-zero width ends the block in front of it
                mine[-1][1:] = gap
                mine.append([0, 0, 0])
            gap = (0, 0)
            mine[-1][0] += n
            eq, x = eq + (n if code == EQ else 0), x + (n if code == X else 0)
            span[1], span[3] = a + n, b + n
        pairs.append((span[0], span[1], span[2], span[3], eq, x, len(blocks), len(mine)) if mine else (0,) * 8)
        blocks += [tuple(m) for m in mine]
    return pairs, blocks


def identities_hold(pairs, blocks):
    for a0, a1, b0, b1, eq, x, first, n in pairs:
        mine = blocks[first:first + n]
        if (a1 - a0, b1 - b0, eq + x) != (sum(s + t for s, t, _ in mine), sum(s + q for s, _, q in mine), sum(s for s, _, _ in mine)):
            return False
        if any(s <= 0 for s, _, _ in mine) or any(t + q <= 0 for _, t, q in mine[:-1]) or (mine and mine[-1][1:] != (0, 0)):
            return False
    return True


def brute_text(pairs, blocks):
    "(text, text_first): per block `size\\tdt\\tdq\\n`, for a pair's last block `size\\n`"
    text, first = b"", [0]
    for p in pairs:
        mine = blocks[p[6]:p[6] + p[7]]
        for j, (s, t, q) in enumerate(mine):
            text += (f"{s}\n" if j == len(mine) - 1 else f"{s}\t{t}\t{q}\n").encode()
        first.append(len(text))
    return text, first


def parse_chain(text):
    """a strict reader of a chain file: [dict(score, tName, tSize, tStrand, tStart, tEnd, qName, qSize, qStrand, qStart, qEnd, id, blocks =
    [(size, dt, dq)])].  ValueError for anything the format does not allow"""
    out, lines, at = [], text.split("\n"), 0
    if text and not text.endswith("\n"):
        raise ValueError("the file does not end with a newline")
    lines = lines[:-1]
    while at < len(lines):
        f = lines[at].split(" ")
        if len(f) != 13 or f[0] != "chain":
            raise ValueError(f"line {at + 1}: no header of 13 fields: {lines[at]!r}")
        names = ("score", "tName", "tSize", "tStrand", "tStart", "tEnd", "qName", "qSize", "qStrand", "qStart", "qEnd", "id")
        c = dict(zip(names, f[1:]))
        for n in ("score", "tSize", "tStart", "tEnd", "qSize", "qStart", "qEnd", "id"):
            if not c[n].isdigit() or (len(c[n]) > 1 and c[n][0] == "0"):
                raise ValueError(f"line {at + 1}: {n} is no plain number")
            c[n] = int(c[n])
        if c["tStrand"] != "+" or c["qStrand"] not in "+-" or len(c["qStrand"]) != 1:
            raise ValueError(f"line {at + 1}: strands")
        if not (c["tStart"] < c["tEnd"] <= c["tSize"] and c["qStart"] < c["qEnd"] <= c["qSize"]):
            raise ValueError(f"line {at + 1}: a span outside its sequence")
        if c["id"] != len(out) + 1:
            raise ValueError(f"line {at + 1}: ids do not count from 1")
        at += 1
        blocks = []
        while True:
            if at >= len(lines):
                raise ValueError("the file ends inside a chain")
            g = lines[at].split("\t")
            if len(g) not in (1, 3) or any(not v.isdigit() or (len(v) > 1 and v[0] == "0") for v in g):
                raise ValueError(f"line {at + 1}: no block line: {lines[at]!r}")
            g = [int(v) for v in g]
            if g[0] <= 0:
                raise ValueError(f"line {at + 1}: a block of size 0")
            at += 1
            if len(g) == 1:
                blocks.append((g[0], 0, 0))
                break
            if g[1] == 0 and g[2] == 0:
                raise ValueError(f"line {at}: a gap line `0 0`")
            blocks.append(tuple(g))
        if at >= len(lines) or lines[at] != "":
            raise ValueError(f"line {at + 1}: no blank line behind the chain")
        at += 1
        if at < len(lines) and lines[at] == "":
            raise ValueError(f"line {at + 1}: more than one blank line")
        if c["tEnd"] - c["tStart"] != sum(s + t for s, t, _ in blocks) or c["qEnd"] - c["qStart"] != sum(s + q for s, _, q in blocks):
            raise ValueError(f"chain {c['id']}: the blocks do not add up to its spans")
        c["blocks"] = blocks
        out.append(c)
    return out


def chain_blocks(c):
    "the blocks of one parsed chain as (tStart, qStart on the chain's query strand, size)"
    t, q, out = c["tStart"], c["qStart"], []
    for s, dt, dq in c["blocks"]:
        out.append((t, q, s))
        t, q = t + s + dt, q + s + dq
    return out


def lift_base(chains, contig, pos):
    """liftOver's rule for one base: every (qName, strand, forward position on the query) to which a block of a chain on `contig` that
    holds target base `pos` maps it; for a `-` chain the block's query coordinates lie on the reverse strand: forward = qSize - 1 - r"""
    out = []
    for c in chains:
        if c["tName"] != contig or not c["tStart"] <= pos < c["tEnd"]:
            continue
        for t, q, s in chain_blocks(c):
            if t <= pos < t + s:
                r = q + pos - t
                out.append((c["qName"], c["qStrand"], c["qSize"] - 1 - r if c["qStrand"] == "-" else r))
    return out


def chains_from_paf(paf_text):
    """the chain file a run must write, from its PAF text alone: the records grouped by (bi, tg, qg) in file order and ordered by ch, the
    seams taken from the coordinates (the target forwards; the query forwards for `+`, on its reverse strand for `-`: both ascend with
    ch), the blocks collected by the definition"""
    groups = {}
    for line in paf_text.splitlines():
        f = line.split("\t")
        tags = {t[:5]: t[5:] for t in f[12:]}
        q_size, q0, q1, flip = int(f[1]), int(f[2]), int(f[3]), f[4] == "-"
        rec = dict(q=f[0], q_size=q_size, flip=flip, t=f[5], t_size=int(f[6]), t0=int(f[7]), ch=int(tags["ch:i:"]), entries=LB.parse_cigar(tags["cg:Z:"]),
                   qs=q_size - q1 if flip else q0)
        groups.setdefault((tags["bi:i:"], tags["tg:Z:"], tags["qg:Z:"]), []).append(rec)
    out, n = [], 0
    for records in groups.values():
        records.sort(key=lambda r: r["ch"])
        cigar, chains, links = [], [], []
        for c, r in enumerate(records):
            len_a = sum(v >> 4 for v in r["entries"] if v & 15 in (EQ, X, D))
            len_b = sum(v >> 4 for v in r["entries"] if v & 15 in (EQ, X, I))
            chains.append({"first": len(cigar), "n_cig": len(r["entries"]), "len_a": len_a, "len_b": len_b})
            links.append({"chain": c, "a0": r["t0"], "b0": r["qs"]})
            cigar += r["entries"]
        links = [l for l, c in zip(links, chains) if c["n_cig"]]
        (a0, a1, b0, b1, eq, x, _, nb), = brute_blocks(cigar, chains, links, [0, len(links)])[0]
        blocks = brute_blocks(cigar, chains, links, [0, len(links)])[1]
        if nb == 0:
            continue
        n += 1
        r = records[0]
        out.append(f"chain {eq} {r['t']} {r['t_size']} + {a0} {a1} {r['q']} {r['q_size']} {'-' if r['flip'] else '+'} {b0} {b1} {n}\n" +
                   brute_text([(a0, a1, b0, b1, eq, x, 0, nb)], blocks)[0].decode() + "\n")
    return "".join(out)
