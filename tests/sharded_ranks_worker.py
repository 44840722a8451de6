"""Worker of test_sharded_counter_with_four_ranks (run under torch.distributed.run: four ranks, gloo, every rank on device 0):
exchange.ShardedCounter as a job uses it, against the oracle, which runs in here on the CPU.  argv: k m b.  Every rank prints
"ok rank <r>"; any mismatch is an AssertionError and a non-zero exit status of the launcher."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.distributed as dist

import sharded_cases as C
import sharded_job as S
from brisk_amd.exchange import ShardedCounter

k, m, b = (int(x) for x in sys.argv[1:4])
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
assert world == 4
dist.init_process_group("gloo")
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
sc = ShardedCounter(k, m, b, rank, world, 0, stream)
batches = [[C.rank_reads(i, r) for r in range(world)] for i in range(len(C.RANK_SHARES))]
everything = [s for batch in batches for share in batch for s in share]
E = S.expect(everything, k, m, b)
default_k31 = (k, m, b) == (31, 15, 14)


def on_device(reads):
    if not reads:
        return torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    return S.to_device(sc.ix, reads)


def gathered(x):
    out = [None] * world
    dist.all_gather_object(out, x)
    return out


# 1. balance() on the rank's reads: cut points at k31 m15 b14 (the same on every rank), none at (31, 11, 4)
mine = [s for batch in batches for s in batch[rank]]
d_packed, d_starts = on_device(mine)
cuts = sc.balance(d_packed, d_starts, len(mine))
if default_k31:
    assert cuts is not None and sc.owner_load["uniform_max_over_mean"] > 1.3, (cuts, sc.owner_load)
    assert cuts[0] == 0 and cuts[-1] == 1 << sc.ix.layout["part_bits"] and cuts == sorted(cuts) and len(cuts) == world + 1
else:
    assert cuts is None and sc.owner_load["uniform_max_over_mean"] <= 1.3, (cuts, sc.owner_load)
assert all(c == cuts for c in gathered(cuts)), "the ranks installed different cut points"

# 2. two count_packed batches with unequal and empty shares; the first outgrows six records a read where the oracle says so
cap0 = C.RANK_SHARES[0][rank] * 6 + 4096
n_rec0 = len(S.oracle_partitions(batches[0][rank], k, m, b)[0]) if batches[0][rank] else 0
if default_k31 and rank == 0:
    assert n_rec0 > cap0, (n_rec0, cap0)  # (26,092 records of 2000 reads against 16,096)
for i, batch in enumerate(batches):
    d_packed, d_starts = on_device(batch[rank])
    sc.count_packed(d_packed, d_starts, len(batch[rank]))
    sc.ix.sync()
    if i == 0:
        assert (sc._cap > cap0) == (n_rec0 > cap0), ("the scan buffers after the first call", sc._cap, cap0, n_rec0)
        assert sc._cap >= n_rec0

# 3. stats and 4. checksums of the whole job
st = sc.stats()
assert (st["nb_kmers"], st["nb_buckets"]) == E.stats, (st, E.stats)
sums = gathered(sc.ix.checksum())
got = (sum(c[0] for c in sums), sum(c[1] for c in sums), sum(c[2] for c in sums) % (1 << 64))
assert got == E.digest, (got, E.digest)
assert sum(1 for c in sums if c[0] * 10 >= got[0]) >= 2, ("fewer than two ranks hold a tenth of the entries", sums)

# 5. get_packed: every rank's own reads, then reads that are not in the index (rank 3 asks for none)
rng = random.Random(900 + rank)
absent = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(0 if rank == 3 else 40 + rank)]
for what, queries in (("own", mine), ("absent", absent)):
    d_packed, d_starts = on_device(queries)
    sums = sc.get_packed(d_packed, d_starts, len(queries))
    stream.synchronize()
    want = E.query(queries) if queries else np.zeros(0, np.uint64)
    assert np.array_equal(sums.cpu().numpy().astype(np.uint64), want), (rank, what)
    if what == "own":
        assert int(want.sum()) > 0
sc.ix.close()
dist.barrier()
os.write(1, b"ok rank %d\n" % rank)  # one write: the ranks share the launcher's pipe
dist.destroy_process_group()
