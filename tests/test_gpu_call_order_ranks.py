"""The exchanges between ranks give their results after any other call (docs/design/04_24_call_order.md, "The exchanges"): case `order`
of tests/multirank_worker.py runs nts_bf_allreduce_and / _groups / _parts and nts_mx_allgather_ex in ONE context per rank, in orders
tests/test_gpu_multirank.py never takes -- a smaller filter after a larger one, dense after sparse and back, one and two contributions
per rank out of the same scratch halves, an exchange 2 between two exchange 1s at list sizes that fall and rise (a list whose largest
position is 2^32 - 1 beside one whose largest is 2^32), a good call behind each of the four refused ones, and two single-rank entries
of tests/call_order_cases.py between exchanges.  World 2 and 3 over the librccl stand-in (processes that share GPU 0), with the
product's piece size and with pieces of 64 KiB; every result against numpy inside the worker."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN = os.path.join(ROOT, "tests", "rccl_standin", "librccl_standin.so")
WORKER = os.path.join(ROOT, "tests", "multirank_worker.py")
# a worker's share: starting Python and a context, some sixty exchanges of at most 3 MB, two catalogue expectations -- seconds; the
# limit is what the ranks of one test may take together before the test gives them up, not what they take (under 2 s)
RANK_SECONDS = 60
# the exported functions of csrc/nts_comm.inc that request scratch -> the call in the worker's `order` case that reaches each
# (tests/test_call_order_cases_host.py reads the sources for them).  nts_mx_allgather is nts_mx_allgather_ex with no slot count.
CALLS = {"nts_bf_allreduce_and": "comm.allreduce_and(", "nts_bf_allreduce_groups": "comm.allreduce_groups(", "nts_bf_allreduce_parts": "comm.allreduce_parts(",
         "nts_mx_allgather_ex": "comm.allgather_minimizers(", "nts_mx_allgather": "comm.allgather_minimizers("}
# what nts_comm_last_sparse says after every exchange 1 of the case, in its order: the five filters (large dense, small dense, large all
# but empty, middle dense, 64 bytes of zeros), groups, parts dense and all but empty, and again; around the exchange 2s; behind each
# refused call; behind each single-rank call
SPARSE = [False, False, True, False, True] + [False, False, True, False] + [False, True] + [False, False, False] + [False, False]
REFUSED = ["a group without a filter", "a gap in a rank's slots", "a repeated genome number", "a list out of record order"]


def ranks(world, tmp_path, **extra):
    "`world` workers of the case on GPU 0 (at most 3 processes beside this one); their JSON lines"
    assert os.path.exists(STANDIN), "tests/rccl_standin/librccl_standin.so is not built (__graft_entry__.build())"
    env = dict(os.environ, PYTHONPATH=ROOT, NTS_RCCL_LIB=STANDIN, **extra)
    id_file = str(tmp_path / f"id_order_{world}")
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), id_file, "order"], env=env, cwd=tmp_path, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = []
    deadline = time.monotonic() + RANK_SECONDS                # one deadline for all ranks: they run side by side
    try:
        for r, p in enumerate(procs):
            so, se = p.communicate(timeout=max(deadline - time.monotonic(), 1))
            assert p.returncode == 0, f"rank {r}: {se[-3000:]}"
            outs.append(json.loads([ln for ln in so.splitlines() if ln.startswith("{")][-1]))
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
    return outs


@pytest.mark.parametrize("piece", [None, "65536"], ids=["product_piece", "piece_64k"])
@pytest.mark.parametrize("world", [2, 3])
def test_exchanges_in_one_context_in_orders_that_rise_and_fall(world, piece, tmp_path):
    outs = ranks(world, tmp_path, **({} if piece is None else {"NTS_COMM_PIECE": piece}))
    assert len(outs) == world
    for o in outs:
        print(o)
        assert o["library"] == STANDIN and o["world"] == world
        assert o["sparse"] == SPARSE, (o["rank"], o["sparse"])
        assert o["refused"] == REFUSED
        x2 = o["exchange2"]                                   # the last L gather: 12 bytes a minimizer where positions fit 32 bits, 16 where not
        assert 0 < x2["packed_bytes"] < x2["unpacked_bytes"] == 20 * (4099 + 1000 + 37)
