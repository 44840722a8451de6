"""Worker of test_sharded_kmers.test_sharded_counter_with_four_ranks (run under torch.distributed.run: four ranks, gloo, every rank
on device 0): exchange.ShardedCounter's per-k-mer get, read profiles, trimming, spectrum, prune and checksum as a job uses them,
against the oracle, which runs in here on the CPU.  argv: k m b.  Every rank prints "ok rank <r>"; any mismatch is an
AssertionError and a non-zero exit status of the launcher."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.distributed as dist

import brisk_amd
import oracle
import sharded_cases as C
import sharded_job as S
import sharded_kmers_job as K
from brisk_amd.exchange import ShardedCounter
from test_kmer_query import assert_slots

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


def on_device(reads):
    if not reads:
        return torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    return S.to_device(sc.ix, reads)


# the job: two count_packed batches with unequal and empty shares, equal ranges
for batch in batches:
    d_packed, d_starts = on_device(batch[rank])
    sc.count_packed(d_packed, d_starts, len(batch[rank]))
    sc.ix.sync()
cnt = np.asarray(E.dump[3])
assert np.array_equal(sc.count_spectrum(), np.bincount(cnt, minlength=256).astype(np.uint64)), "count_spectrum"
assert sc.checksum() == E.digest, "checksum"

queries = K.rank_queries(rank)
n = len(queries)
want, alts, base = K.expected(everything, queries, k, m, b)
d_packed, d_starts = on_device(queries)


def slots_now():
    t = sc.get_kmers_packed(d_packed, d_starts, n)
    stream.synchronize()
    return t.cpu().numpy().view(np.uint16)


# 1. get_kmers_packed
got = slots_now()
assert_slots(got, want, alts, (rank, "get_kmers_packed"))
assert (want != 0).any() and (want == 0).any()
truth = K.resolved(want, alts, got)

# 2. read_profile_packed, 256 reads a batch: two agreed batches, rank 2 idle in the second
prof = sc.read_profile_packed(d_packed, d_starts, n, solid_min=2, batch_reads=K.RANK_BATCH_READS)
stream.synchronize()
want_prof = K.expected_profile(truth, base, 2)
K.assert_same_records(prof.cpu().numpy().reshape(-1).view(brisk_amd.READ_PROFILE_DTYPE)[:n], want_prof, (rank, "read_profile_packed"))

# 3. trim_packed with the solid_run rule: the kept intervals, where they start in the output, which reads they are, their nucleotides
rule = brisk_amd.select_rule("solid_run")
iv = brisk_amd.intervals_from_profile(want_prof, k, rule)
words = d_packed.numel()
d_out = torch.zeros(words, dtype=torch.int32, device=dev)
d_out_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
d_out_index = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
torch.cuda.synchronize()
n_out, n_nts = sc.trim_packed(d_packed, d_starts, n, d_out.data_ptr(), words, d_out_starts.data_ptr(), d_out_index.data_ptr(), solid_min=2, rule=rule,
                              batch_reads=K.RANK_BATCH_READS)
kept = np.nonzero(iv["len"] > 0)[0]
assert (n_out, n_nts) == (len(kept), int(iv["len"].astype(np.int64).sum())), (rank, "trim_packed", n_out, n_nts)
assert 0 < len(kept) < n
assert np.array_equal(d_out_index[:n_out].cpu().numpy(), kept)
assert np.array_equal(d_out_starts[:n_out + 1].cpu().numpy(), np.concatenate([[0], np.cumsum(iv["len"][kept].astype(np.int64))]))
d_bases = torch.zeros(max(n_nts, 1), dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
sc.ix.unpack_ascii(d_out.data_ptr(), 0, n_nts, d_bases.data_ptr())
sc.ix.sync()
assert d_bases[:n_nts].cpu().numpy().tobytes().decode() == "".join(queries[i][iv["start"][i]:iv["start"][i] + iv["len"][i]] for i in kept), (rank, "trimmed reads")

# 4. prune(2, 255) on every owner; afterwards the index is the oracle's without its entries of count 0 and 1
removed = sc.prune(2, 255)
assert removed == int((cnt < 2).sum()), (rank, "prune", removed)
keep = cnt >= 2
assert sc.checksum() == oracle.digest(*[np.asarray(a)[keep] for a in E.dump]), "checksum after the prune"
gone = lambda v: np.where((v & 0xff) < 2, 0, v).astype(np.uint16)
assert_slots(slots_now(), gone(want), [(s, e, gone(v)) for s, e, v in alts], (rank, "get_kmers_packed after the prune"))
sc.ix.close()
dist.barrier()
os.write(1, b"ok rank %d\n" % rank)  # one write: the ranks share the launcher's pipe
dist.destroy_process_group()
