"""The sharded per-k-mer get on ONE MI355X: what rank 0 of N does, stage by stage (the exchange itself cannot be measured here;
its bytes are printed), next to the unsharded calls on the same reads.

  python tools/sharded_kmers_bench.py [N] [reads_per_rank] [part_bits]     defaults: 8 owners, 6.25 M reads a rank, 2^27 partitions

k63 m21 b14, the bench's synthetic reads (150 nt).  The index holds all N x reads_per_rank reads; every rank asks for every k-mer of
its own reads.  Rank 0 is played in full -- as asker: scan_kmers, route_tagged, record_kmers, place_answers, profile_slots; as
owner: record_kmers and answer_records over what the N peers route to it (each peer's share is scanned here in turn, as
tools/owner_emulation.py does).  The answers of the other owners are not computed: place_answers moves a buffer of the right size.
Wall times include the calls' host synchronisations; the median of three repetitions after a warm-up is printed, and one JSON line at the end."""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import brisk_amd

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8
Q = int(sys.argv[2]) if len(sys.argv) > 2 else 6_250_000
PB = int(sys.argv[3]) if len(sys.argv) > 3 else 27
L, k, m, b, REPS = 150, 63, 21, 14, 3
G = N * Q * L // 15
dev = torch.device("cuda", 0)


def synth(ix, first, n):
    d_packed = torch.zeros((n * L + 15) // 16 + 4, dtype=torch.int32, device=dev)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ix.synth_reads(G, first, n, L, d_packed.data_ptr(), d_starts.data_ptr())
    ix.sync()
    return d_packed, d_starts


def timed(fn):
    ms, r = [], fn()  # (a warm-up: scratch buffers grow and code objects load in the first call)
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), r


ix = brisk_amd.BriskHip(k, m, b, owner_rank=0, n_owners=N, part_bits=PB)
W = ix.record_words
cap = Q * 6 + 4096
rec = torch.empty(cap * W, dtype=torch.int64, device=dev)
out = torch.empty(cap * W, dtype=torch.int64, device=dev)
tags = torch.empty(cap, dtype=torch.int32, device=dev)
tags_out = torch.empty(cap, dtype=torch.int32, device=dev)
anchors = torch.empty(cap, dtype=torch.int64, device=dev)
inbox = torch.empty((cap + cap // 2) * W, dtype=torch.int64, device=dev)
torch.cuda.synchronize()
rows, n_in, mine = {}, 0, None
for peer in range(N - 1, -1, -1):  # rank 0's own share last: its buffers are what the asker's stages below read
    d_packed, d_starts = synth(ix, peer * Q, Q)
    if peer == 0:
        rows["scan_kmers"], (n_rec, n_slots) = timed(lambda: ix.scan_kmers(d_packed.data_ptr(), d_starts.data_ptr(), Q, rec.data_ptr(), tags.data_ptr(), anchors.data_ptr(), cap))
        rows["route_tagged"], counts = timed(lambda: ix.route_tagged(rec.data_ptr(), tags.data_ptr(), n_rec, out.data_ptr(), tags_out.data_ptr()))
        mine = (d_packed, d_starts)
    else:
        n_rec, _ = ix.scan_kmers(d_packed.data_ptr(), d_starts.data_ptr(), Q, rec.data_ptr(), tags.data_ptr(), anchors.data_ptr(), cap)
        counts = ix.route_tagged(rec.data_ptr(), tags.data_ptr(), n_rec, out.data_ptr(), tags_out.data_ptr())
    c0 = int(counts[0])
    inbox[n_in * W:(n_in + c0) * W].copy_(out[: c0 * W])
    n_in += c0
torch.cuda.synchronize()
ix.insert_records(inbox.data_ptr(), n_in)  # owner 0's share of the index: the records of its range from all N ranks
ix.sync()
offs_out = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
offs_in = torch.empty(n_in + 1, dtype=torch.int64, device=dev)
torch.cuda.synchronize()
rows["record_kmers (asker)"], _ = timed(lambda: ix.record_kmers(out.data_ptr(), n_rec, offs_out.data_ptr()))
rows["record_kmers (owner)"], _ = timed(lambda: ix.record_kmers(inbox.data_ptr(), n_in, offs_in.data_ptr()))
n_ans_in = int(offs_in[n_in].item())
answers = torch.empty(max(n_ans_in, n_slots, 1), dtype=torch.int16, device=dev)
torch.cuda.synchronize()
rows["answer_records"], _ = timed(lambda: ix.answer_records(inbox.data_ptr(), n_in, offs_in.data_ptr(), answers.data_ptr()))
found = int((answers[:n_ans_in] != 0).sum().item())
assert found == n_ans_in, "every k-mer asked of owner 0 was inserted there"
slots = torch.empty(n_slots, dtype=torch.int16, device=dev)
prof = torch.empty(Q * 32, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
rows["place_answers"], _ = timed(lambda: ix.place_answers(out.data_ptr(), tags_out.data_ptr(), anchors.data_ptr(), n_rec, offs_out.data_ptr(), answers.data_ptr(), slots.data_ptr(), n_slots))
rows["profile_slots"], _ = timed(lambda: ix.profile_slots(slots.data_ptr(), mine[1].data_ptr(), Q, prof.data_ptr(), 2))
sent = n_rec - int(counts[0])
bytes_out, bytes_back = sent * W * 8, 2 * int((offs_out[n_rec] - offs_out[int(counts[0])]).item())
print(f"rank 0 of {N}, k{k} m{m} b{b}, 2^{ix.layout['part_bits']} partitions, {Q} reads a rank: {n_rec} records and {n_slots} slots asked, {n_in} records / {n_ans_in} answers owed ({found} present)")
for name, ms in rows.items():
    print(f"  {name:24s} {ms:9.3f} ms wall")
total = sum(rows.values())
print(f"  {'sum of the stages':24s} {total:9.3f} ms   (without profile_slots: {total - rows['profile_slots']:.3f})")
print(f"  exchange (not measured): {bytes_out / 1e6:.1f} MB of records out, {bytes_back / 1e6:.1f} MB of answers back per rank; >= {(bytes_out + bytes_back) / (7 * 153e9) * 1e3:.3f} ms at 7 x 153 GB/s")
ix.close()
del rec, out, tags, tags_out, anchors, inbox, answers, offs_in, offs_out

# the unsharded calls: one index of all N x Q reads, asked for the rank's reads and for the whole job's
one = brisk_amd.BriskHip(k, m, b)
allp, alls = synth(one, 0, N * Q)
one.insert_packed(allp.data_ptr(), alls.data_ptr(), N * Q)
one.sync()
big = torch.empty(N * n_slots, dtype=torch.int16, device=dev)
bigprof = torch.empty(N * Q * 32, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
res = {}
for what, n in (("rank's reads", Q), ("whole job", N * Q)):
    res[what] = (timed(lambda: one.get_kmers_packed(allp.data_ptr(), alls.data_ptr(), n, big.data_ptr()))[0],
                 timed(lambda: one.read_profile_packed(allp.data_ptr(), alls.data_ptr(), n, bigprof.data_ptr(), 2))[0])
    print(f"unsharded, {what} ({n} reads): get_kmers_packed {res[what][0]:.3f} ms, read_profile_packed {res[what][1]:.3f} ms")
print(json.dumps({"n_owners": N, "reads_per_rank": Q, "part_bits": PB, "stages_ms": {n: round(v, 3) for n, v in rows.items()}, "sum_ms": round(total, 3),
                  "bytes_out": bytes_out, "bytes_back": bytes_back, "unsharded_rank_ms": [round(v, 3) for v in res["rank's reads"]],
                  "unsharded_job_ms": [round(v, 3) for v in res["whole job"]]}))
