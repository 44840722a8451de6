// brisk_count -- this repo's own small k-mer counter over the facade / C-ABI (not the reference's
// apps/counter.cpp, which compiles unchanged against brisk_amd/include and is built by the tests).
//   brisk_count --facade FASTA k m b [dump.txt]   per-call API: SuperKmerEnumerator + Brisk<uint8_t>
//   brisk_count --bulk   FASTA k m b [dump.txt]   bulk C-ABI: brisk_hip_insert_reads, FASTA or FASTA.gz streamed in batches; a file whose first
//                                                 inflated byte is '@' is FASTQ (plain or .gz) and goes through brisk_hip_insert_raw_reads
//   brisk_count --mixed  FASTA k m b              BASELINE config #5's protocol (apps/counter.cpp:197-227,314-346): one thread streams the
//                                                 file into brisk_hip_insert_reads while a second thread issues brisk_hip_get_reads on
//                                                 the first reads of batches that are already in; prints what every get saw
// --bulk only, anywhere on the command line (taken out before the positional arguments are read):
//   --min-qual Q [--qual-base 33|64]   FASTQ input only (the main input and the FILE of --merge / --subtract / --intersect / --filter-joint /
//                    --joint): a base whose quality is below Q (0..93, default 0: no cut) is cut like an N, on the device; the quality
//                    characters are Phred+33 (default) or Phred+64.  One line on stderr per FASTQ file carries the intake's stats.
//                    Exit status 2 when no input is FASTQ.  --profile and --extract read the input again as FASTA: with a FASTQ main
//                    input they exit 2 (--extract takes one with --paired, below)
//   --histo FILE     the count spectrum (brisk_hip_count_spectrum): 256 lines "count<TAB>entries", empty bins included
//   --saturate       counts stop at 255 instead of wrapping (brisk_hip_options.count_mode = BRISK_HIP_COUNTS_SATURATE): the index, and the
//                    second index of --merge / --subtract / --intersect FILE, are created in that mode; --load FILE (or a set operation's
//                    FILE) of a snapshot of the other mode fails with the library's message.  The --histo file then starts with a
//                    "#" comment line saying so, and its last line is "255+<TAB>entries": the entries seen 255 times or more
//   --full-minimizers   full-width minimizers (brisk_hip_options.minimizer_mode = BRISK_HIP_MINIMIZER_FULL): the re-scan of a k-mer sees all
//                    of it at k > 32 too, so that one canonical k-mer is one entry (the reference's truncation splits it among several); the
//                    index and the second index of a set operation are created in that mode, and a snapshot of the other mode is refused
//                    with the library's message.  --bulk only: --facade and --mixed stay the reference's
//   --degrees FILE   the degree spectrum of the index as a de Bruijn graph (brisk_hip_degree_spectrum, nodes: count >= --min-count): five lines
//                    "n0<TAB>..<TAB>n4" -- line `left`, column `right` -- and a line "below<TAB>n" for the entries under the threshold; the figures
//                    (nodes, edge ends, isolated, dead ends, simple, branching) go to stderr.  At k > 32 give --full-minimizers.
//   --prune-degrees L:R[,L:R...]   remove the nodes (--min-count <= count <= --max-count) with L neighbours on the left and R on the right
//                    (brisk_hip_prune_degrees; 0:0 the isolated ones, 0:1,1:0 the tips' ends); one line on stderr says how many went.  Both run where
//                    --histo runs, --degrees first: after load, the set operations and a count prune
//   --min-count N / --max-count N   the dump and the KFF file hold only the entries with N <= count (<= N): brisk_hip_enumerate_range
//   --merge FILE / --subtract FILE / --intersect FILE   each at most once, applied in that order: FILE is counted into a second index with
//                    the same parameters and combined with the first on the device (brisk_hip_merge / _subtract / _intersect, counts of
//                    the first kept by --intersect) before --histo, --min-count / --max-count and the dump take effect; one line on stderr
//                    per operation with the entries added / removed.  A FILE that is a snapshot (recognised by its magic) is loaded
//                    (brisk_hip_load) instead of counted
//   --filter-joint FILE --window SLO:SHI:OLO:OHI[:absent]   after --merge / --subtract / --intersect and before the prune: FILE becomes a
//                    second index as theirs does, and the first keeps the entries whose count is in SLO..SHI and whose count in the second
//                    is in OLO..OHI -- with ":absent" also those the second does not hold (brisk_hip_filter_joint); OLO > OHI: only those
//   --joint FILE --joint-histo OUT   after load, set operations and a --min-count / --max-count prune: the joint count spectrum of the final
//                    index and FILE's (brisk_hip_joint_spectrum): one line "state_self<TAB>state_other<TAB>entries" per non-zero bin,
//                    ascending by self, then by other; a state is a stored count, or -1 for "not in that index", which sorts last
//   --load FILE      start from the snapshot FILE (brisk_hip_load, slices with room to grow) instead of the empty index, and count FASTA on
//                    top; a FASTA of "-" means no reads.  k m b must be the file's (exit status 2 otherwise)
//   --save FILE      write the final index -- after counting, the set operations and, if given, --min-count / --max-count applied as
//                    brisk_hip_prune -- as a snapshot (brisk_hip_save)
//   --extract FILE --rule trim|median:LO:HI|present:LO:HI [--solid N] [--min-len L]
//                    after load, set operations and prune (where --profile runs): the reads of the input again, against the final index,
//                    through brisk_hip_trim_reads; FILE receives what the rule keeps of every kept read as FASTA, the header
//                    ">read_index start len".  trim (the default): the stretch covered by the first longest run of k-mers with count
//                    >= N (--solid, default 2); median:LO:HI: the whole read when LO <= its median count <= HI; present:LO:HI: when
//                    LO <= the permille of its k-mers that are in the index <= HI.  --min-len L: at least L nucleotides (default k)
//   --extract FILE --rule split [--solid N] [--min-len L]
//                    the same reads through brisk_hip_split_reads: a read is cut at its weak k-mers, and every run of k-mers with count >= N
//                    that covers at least L nucleotides (default k) is a record of its own, ">read_index start len", ordered by read, then
//                    by start; the counters of brisk_hip_split_stats go to stderr.  Not with --paired (exit status 2)
//   --extract FILE --rule correct [--solid N] [--min-cover C]
//                    the same reads through brisk_hip_correct_reads: every read leaves whole, as one record ">read_index n_corrected", with
//                    its isolated substitutions repaired (a run of weak k-mers that one substitution explains, exactly one other base
//                    making every k-mer of the run solid); C: the fewest weak k-mers a run at a read's edge may have (default k); the
//                    counters of brisk_hip_correct_stats go to stderr.  Not with --paired (exit status 2)
//   --paired [--mate FILE] [--pair-mode each|all|any]
//                    the input holds paired reads, one record a read: interleaved (records 2p and 2p + 1 are the mates of pair p), or,
//                    with --mate FILE, record i of the input and record i of FILE (of the same kind, FASTA or FASTQ) are a pair.  A
//                    record count that is odd, or differs between the two files, exits 2.  Pairing never changes the index: the reads
//                    are counted exactly as unpaired ones (FILE after the input).  With --extract PREFIX three files are written,
//                    PREFIX.1.fa and PREFIX.2.fa (the mates of intact pairs, line by line in step) and PREFIX.s.fa (the surviving mate
//                    of a broken pair), headers ">pair_index/1 start len" and ">pair_index/2 start len", start relative to the input
//                    read; the pair counts go to stderr on one line.  --pair-mode (default each): each -- mates are judged alone; all
//                    -- a pair stays only when both mates do; any -- when either mate passes the rule both are kept whole.  FASTA
//                    records must be clean (ACGTacgt only, else exit 2, like the counts before anything is counted) and go through brisk_hip_trim_pairs_reads; FASTQ records go
//                    through brisk_hip_clean_pairs_reads with --min-qual / --qual-base: the first longest clean fragment of a read,
//                    cut again by the rule -- the one case in which --extract takes a FASTQ input
// Prints nb_kmers / nb_buckets / sum of counts (of the entries dumped); optionally dumps "KMER idx count" lines (dump.txt, "-" for none) and
// writes the index as a KFF file (a 7th argument: BriskWriter in --facade mode, brisk_write_kff in --bulk mode).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <atomic>
#include <chrono>
#include <iostream>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "Brisk.hpp"
#include "brisk_fasta.hpp"
#include "brisk_fastq.hpp"
#include "writer.hpp"

// a snapshot file is told from a FASTA by its first eight bytes
static bool is_snapshot(const char* path) {
    char magic[8] = {0};
    std::ifstream in(path, std::ios::binary);
    return in.read(magic, 8) && !memcmp(magic, "BRSKSNP1", 8);
}
// FILE into `h` for --load / --merge / --subtract / --intersect.  0 fine, 1 failed, 2 the file's k m b are not the command line's.
static int load_snapshot(brisk_hip_index* h, const char* opt, const char* path, uint8_t k, uint8_t m, uint8_t b, uint32_t flags) {
    brisk_hip_snapshot_info info{};
    info.struct_size = sizeof info;
    if (brisk_hip_snapshot_info_read(path, &info) != BRISK_HIP_OK) {
        std::cerr << opt << " " << path << ": not a readable snapshot" << std::endl;
        return 1;
    }
    if (info.k != k || info.m != m || info.b != b) {
        std::cerr << opt << " " << path << ": the snapshot has k " << info.k << " m " << info.m << " b " << info.b << ", the command line k " << (int)k << " m " << (int)m << " b "
                  << (int)b << std::endl;
        return 2;
    }
    uint64_t n = 0;
    if (brisk_hip_load(h, path, flags, &n) != BRISK_HIP_OK) {
        std::cerr << opt << " " << path << ": " << brisk_hip_last_error(h) << std::endl;
        return 1;
    }
    std::cerr << (opt + 2) << " " << path << ": " << n << " entries loaded" << std::endl;
    return 0;
}

static bool is_fastq(const char* path) { return strcmp(path, "-") && !is_snapshot(path) && first_inflated_byte(path) == '@'; }
// a FASTQ file into `h`: whole records as they are to brisk_hip_insert_raw_reads, which cuts them on the device; one stderr line with
// the stats.  0 fine, 1 failed.  *produce_s / *wait_s (may be null): the reader thread's seconds, and the seconds spent waiting for it
static int count_fastq(brisk_hip_index* h, const char* path, const brisk_hip_intake_rule& rule, size_t batch_bases, double* produce_s = nullptr, double* wait_s = nullptr) {
    brisk_hip_intake_stats total{};
    try {
        FastqBatcher batches(path, batch_bases);
        FastqBatch bt;
        while (batches.next(bt)) {
            brisk_hip_intake_stats st{};
            if (brisk_hip_insert_raw_reads(h, bt.bases.data(), rule.min_qual ? bt.quals.data() : nullptr, bt.offs.data(), bt.size(), &rule, &st) != BRISK_HIP_OK) {
                std::cerr << path << ": " << brisk_hip_last_error(h) << std::endl;
                return 1;
            }
            const uint64_t* v = (const uint64_t*)&st;
            for (size_t i = 0; i < sizeof st / 8; i++) ((uint64_t*)&total)[i] += v[i];
        }
        if (produce_s) *produce_s = batches.produce_seconds();
        if (wait_s) *wait_s = batches.consumer_wait_seconds();
    } catch (const std::exception& e) {
        std::cerr << path << ": " << e.what() << std::endl;
        return 1;
    }
    std::cerr << "fastq " << path << ": n_reads=" << total.n_reads << " n_reads_kept=" << total.n_reads_kept << " n_fragments=" << total.n_fragments << " n_bases_in=" << total.n_bases_in
              << " n_nts=" << total.n_nts << " n_cut_base=" << total.n_cut_base << " n_cut_qual=" << total.n_cut_qual << " n_short=" << total.n_short << std::endl;
    return 0;
}

// --paired: a file read record by record, one record a read, nothing cleaned.  FASTA: the lines of a record concatenated;
// FASTQ: brisk_fastq.hpp's strict four-line records.
class RecordReader {
  public:
    RecordReader(const char* path, bool fastq) : fastq_(fastq) {
        if (fastq) {
            fq_.reset(new FastqReader(path));
        } else {
            gz_ = gzopen(path, "rb");
            if (!gz_) throw std::runtime_error(std::string("cannot open ") + path);
            gzbuffer(gz_, 1 << 20);
            line_.resize(1 << 16);
        }
    }
    ~RecordReader() {
        if (gz_) gzclose(gz_);
    }
    RecordReader(const RecordReader&) = delete;
    RecordReader& operator=(const RecordReader&) = delete;
    // the next record's bases appended to `bases` (its qualities to `quals`, FASTQ only); false at the end of the file
    bool next(std::string& bases, std::string& quals) {
        if (fastq_) {
            one_.clear();
            if (!fq_->fill(one_, 0)) return false;
            bases += one_.bases;
            quals += one_.quals;
            return true;
        }
        if (!have_header_ && !skip_to_header()) return false;
        have_header_ = false;
        for (;;) {  // sequence lines up to the next header
            bool whole = false;
            size_t n = 0;
            if (!read_piece(&n, &whole)) return true;
            if (at_line_start_ && n && line_[0] == '>') {
                have_header_ = true;
                finish_line(whole);
                return true;
            }
            bases.append(line_.data(), n);
            at_line_start_ = whole;
        }
    }

  private:
    // up to a buffer of the current line, without '\n' and '\r'; *whole: the line ended here.  false at the end of the file
    bool read_piece(size_t* n, bool* whole) {
        if (!gzgets(gz_, &line_[0], (int)line_.size())) return false;
        size_t len = strlen(line_.data());
        *whole = len && line_[len - 1] == '\n';
        while (len && (line_[len - 1] == '\n' || line_[len - 1] == '\r')) len--;
        *n = len;
        return true;
    }
    void finish_line(bool whole) {  // the rest of a header line
        size_t n = 0;
        while (!whole && read_piece(&n, &whole)) {
        }
        at_line_start_ = true;
    }
    bool skip_to_header() {  // the file's first record
        for (;;) {
            bool whole = false;
            size_t n = 0;
            if (!read_piece(&n, &whole)) return false;
            const bool header = at_line_start_ && n && line_[0] == '>';
            at_line_start_ = whole;
            if (header) {
                finish_line(whole);
                return true;
            }
        }
    }
    bool fastq_;
    std::unique_ptr<FastqReader> fq_;
    FastqBatch one_;
    gzFile gz_ = nullptr;
    std::string line_;
    bool have_header_ = false, at_line_start_ = true;
};

// the records of a file; *dirty (FASTA: trim_pairs takes clean reads): the first record that holds a byte that is no base, ~0 none
static uint64_t count_records(const char* path, bool fastq, uint64_t* dirty) {
    RecordReader rd(path, fastq);
    std::string bases, quals;
    uint64_t n = 0;
    *dirty = ~0ull;
    for (; rd.next(bases, quals); n++) {
        if (!fastq && *dirty == ~0ull && (bases.find_first_not_of("ACGTacgt") != std::string::npos)) *dirty = n;
        bases.clear();
        quals.clear();
    }
    return n;
}

// --paired --extract PREFIX: the reads again, pair by pair, against the final index; intact pairs to PREFIX.1.fa / PREFIX.2.fa, singles
// to PREFIX.s.fa.  0 fine, else the exit status.
static int extract_paired(brisk_hip_index* h, const char* main_file, const char* mate_file, bool fastq, const char* prefix, const brisk_hip_select_rule& rule, uint32_t solid,
                          const brisk_hip_intake_rule& intake, uint32_t pair_mode, size_t batch_bases) {
    RecordReader rd1(main_file, fastq);
    std::unique_ptr<RecordReader> rd2(mate_file ? new RecordReader(mate_file, fastq) : nullptr);
    const std::string names[3] = {std::string(prefix) + ".1.fa", std::string(prefix) + ".2.fa", std::string(prefix) + ".s.fa"};
    std::ofstream out[3];
    for (int i = 0; i < 3; i++) out[i].open(names[i]);
    brisk_hip_pair_counts total{};
    brisk_hip_intake_stats stats{};
    std::string bases, quals;
    std::vector<uint64_t> offs;
    std::vector<brisk_hip_read_interval> ivs;
    uint64_t pair_index = 0;
    for (bool more = true; more;) {
        bases.clear();
        quals.clear();
        offs.assign(1, 0);
        while (bases.size() < batch_bases) {  // whole pairs
            if (!rd1.next(bases, quals)) {
                more = false;
                break;
            }
            offs.push_back(bases.size());
            if (!(rd2 ? rd2->next(bases, quals) : rd1.next(bases, quals))) {
                std::cerr << "--paired: the input ends inside a pair" << std::endl;
                return 2;
            }
            offs.push_back(bases.size());
        }
        const uint64_t n = offs.size() - 1;
        if (!n) break;
        ivs.resize(n);
        brisk_hip_pair_counts pc{};
        int rc;
        if (fastq) {
            brisk_hip_intake_stats st{};
            rc = brisk_hip_clean_pairs_reads(h, bases.data(), intake.min_qual ? quals.data() : nullptr, offs.data(), n, &intake, &rule, solid, pair_mode, ivs.data(), &pc, &st);
            for (size_t i = 0; i < sizeof st / 8; i++) ((uint64_t*)&stats)[i] += ((const uint64_t*)&st)[i];
        } else {  // (the records are clean: main() has looked at every one before anything was counted)
            rc = brisk_hip_trim_pairs_reads(h, bases.data(), offs.data(), n, solid, &rule, pair_mode, ivs.data(), &pc);
        }
        if (rc != BRISK_HIP_OK) {
            std::cerr << "--extract: " << brisk_hip_last_error(h) << std::endl;
            return 1;
        }
        for (size_t i = 0; i < sizeof pc / 8; i++) ((uint64_t*)&total)[i] += ((const uint64_t*)&pc)[i];
        for (uint64_t p = 0; p < n / 2; p++, pair_index++) {
            const bool both = ivs[2 * p].len && ivs[2 * p + 1].len;
            for (int mate = 0; mate < 2; mate++) {
                const brisk_hip_read_interval v = ivs[2 * p + mate];
                if (!v.len) continue;
                std::ofstream& o = out[both ? mate : 2];
                o << ">" << pair_index << "/" << (mate + 1) << " " << v.start << " " << v.len << "\n";
                o.write(bases.data() + offs[2 * p + mate] + v.start, v.len);
                o << "\n";
            }
        }
    }
    for (int i = 0; i < 3; i++) {
        out[i].close();
        if (!out[i]) {
            std::cerr << "--extract " << names[i] << ": write failed" << std::endl;
            return 1;
        }
    }
    if (fastq)
        std::cerr << "clean " << main_file << ": n_reads=" << stats.n_reads << " n_reads_kept=" << stats.n_reads_kept << " n_fragments=" << stats.n_fragments << " n_bases_in=" << stats.n_bases_in
                  << " n_nts=" << stats.n_nts << " n_cut_base=" << stats.n_cut_base << " n_cut_qual=" << stats.n_cut_qual << " n_short=" << stats.n_short << std::endl;
    std::cerr << "pairs " << prefix << ": n_pairs_in=" << total.n_pairs_in << " n_pairs_kept=" << total.n_pairs_kept << " n_single_first=" << total.n_single_first
              << " n_single_second=" << total.n_single_second << " n_pairs_dropped=" << total.n_pairs_dropped << " n_nts_pairs=" << total.n_nts_pairs << " n_nts_singles=" << total.n_nts_singles
              << std::endl;
    return 0;
}

static std::vector<std::string> read_fasta(const char* path) {
    std::vector<std::string> out;
    FastaReader rd(path);
    FastaBatch b;
    b.clear();
    while (rd.fill(b, (size_t)1 << 26)) {
        if (rd.done()) break;
    }
    for (size_t i = 0; i < b.size(); i++) out.push_back(b.flat.substr(b.offs[i], b.offs[i + 1] - b.offs[i]));
    return out;
}

// --mixed: concurrent insert + get on ONE handle from two host threads (include/brisk_hip.h, "Threads").
// Output, one line each: "batch J N" (batch J of N reads is in), "get J s0 s1 ..." (the per-read sums a get of batch J's
// first reads returned while later batches were being inserted), "final J s0 ..." (the same get after the last batch),
// "digest ENTRIES SUM DIGEST" (brisk_hip_checksum of the final index).
static int run_mixed(const char* path, uint8_t k, uint8_t m, uint8_t b, const double* coef, size_t batch_bases) {
    const size_t sample_reads = getenv("BRISK_MIXED_SAMPLE") ? (size_t)atoll(getenv("BRISK_MIXED_SAMPLE")) : 50;
    brisk_hip_options o{};
    o.struct_size = sizeof o;
    brisk_hip_index* h = nullptr;
    if (brisk_hip_create(&h, k, m, b, 1, coef, &o) != BRISK_HIP_OK) return 1;
    struct Sample {
        std::string flat;
        std::vector<uint64_t> offs;
    };
    std::mutex mu;
    std::vector<Sample> samples;  // sample j = the first reads of batch j, published once batch j is in
    std::vector<std::string> log;
    std::atomic<bool> done{false}, failed{false};
    auto query = [&](size_t j, const char* tag) {
        Sample s;
        {
            std::lock_guard<std::mutex> g(mu);
            s = samples[j];
        }
        std::vector<uint64_t> sums(s.offs.size() - 1);
        if (brisk_hip_get_reads(h, s.flat.data(), s.offs.data(), sums.size(), sums.data()) != BRISK_HIP_OK) {
            failed = true;
            return;
        }
        std::string line = std::string(tag) + " " + std::to_string(j);
        for (uint64_t v : sums) line += " " + std::to_string(v);
        std::lock_guard<std::mutex> g(mu);
        log.push_back(line);
    };
    std::thread getter([&]() {  // keeps asking about batches that are in -- the newest one first, then all of them in turn
        size_t newest_asked = (size_t)-1, turn = 0, asked = 0;
        const size_t max_gets = getenv("BRISK_MIXED_MAX_GETS") ? (size_t)atoll(getenv("BRISK_MIXED_MAX_GETS")) : 2000;
        while (!done && !failed && asked < max_gets) {
            size_t have;
            {
                std::lock_guard<std::mutex> g(mu);
                have = samples.size();
            }
            if (have == 0) {
                std::this_thread::yield();
                continue;
            }
            size_t which = turn++ % have;
            if (have - 1 != newest_asked) which = newest_asked = have - 1;
            query(which, "get");
            asked++;
        }
    });
    FastaBatcher batches(path, batch_bases);
    FastaBatch bt;
    size_t j = 0;
    while (!failed && batches.next(bt)) {
        if (brisk_hip_insert_reads(h, bt.flat.data(), bt.offs.data(), bt.size()) != BRISK_HIP_OK) {
            std::cerr << brisk_hip_last_error(h) << std::endl;
            failed = true;
            break;
        }
        Sample s;
        const size_t ns = std::min(sample_reads, bt.size());
        s.flat = bt.flat.substr(0, bt.offs[ns]);
        s.offs.assign(bt.offs.begin(), bt.offs.begin() + ns + 1);
        std::lock_guard<std::mutex> g(mu);
        samples.push_back(s);
        log.push_back("batch " + std::to_string(j++) + " " + std::to_string(bt.size()));
    }
    done = true;
    getter.join();
    for (size_t q = 0; q < samples.size() && !failed; q++) query(q, "final");
    uint64_t ck[3] = {0, 0, 0};
    if (!failed && brisk_hip_checksum(h, ck) != BRISK_HIP_OK) failed = true;
    brisk_hip_destroy(h);
    for (const std::string& l : log) std::cout << l << "\n";
    std::cout << "digest " << ck[0] << " " << ck[1] << " " << ck[2] << std::endl;
    return failed ? 1 : 0;
}

int main(int argc_in, char** argv_in) {
    // named options first: what is left is the positional command line as it always was
    std::vector<char*> args;
    const char* histo = nullptr;
    const char* degrees_file = nullptr;
    const char* prune_degrees_text = nullptr;
    uint32_t degree_mask = 0;
    const char* save_file = nullptr;
    const char* load_file = nullptr;
    const char* profile_file = nullptr;
    const char* extract_file = nullptr;
    const char* rule_text = nullptr;
    long min_len = 0;
    long min_cover = -1;  // --min-cover C of --rule correct (-1: not given; 0: k)
    long min_qual = 0, qual_base = 33;
    bool have_qual = false;
    long min_count = 0, max_count = 255, solid = 2;
    bool have_solid = false;
    bool have_range = false;
    bool saturate = false;
    bool full_minimizers = false;
    bool paired = false;
    const char* mate_file = nullptr;
    const char* pair_mode_text = nullptr;
    const char* const setop_names[3] = {"--merge", "--subtract", "--intersect"};  // in the order they are applied
    const char* setop_file[3] = {nullptr, nullptr, nullptr};
    const char* joint_file = nullptr;
    const char* joint_histo = nullptr;
    const char* filter_joint_file = nullptr;
    const char* window_text = nullptr;
    static const char* const usage =
        "usage: brisk_count --facade|--bulk|--mixed FASTA k m b [dump.txt [out.kff]]  (--bulk: [--saturate] [--full-minimizers] [--histo FILE] [--degrees FILE] [--prune-degrees L:R[,L:R...]] [--min-count N] [--max-count N] [--merge FILE] "
        "[--subtract FILE] [--intersect FILE] [--filter-joint FILE --window SLO:SHI:OLO:OHI[:absent]] [--joint FILE --joint-histo OUT] [--load SNAPSHOT] [--save SNAPSHOT] [--profile FILE [--solid N]] [--min-qual Q] [--qual-base 33|64] "
        "[--extract FILE --rule trim|median:LO:HI|present:LO:HI [--solid N] [--min-len L]] [--paired [--mate FILE] [--pair-mode each|all|any]]; FASTA \"-\": no reads; a FILE may be a snapshot; an input that starts with '@' is FASTQ)\n"
        "  --min-qual Q   FASTQ input: a base of quality below Q (0..93) is cut like an N, on the device; --qual-base 33|64 (default 33)\n"
        "  --paired   one record a read, interleaved or zipped with --mate FILE; --extract PREFIX then writes PREFIX.1.fa PREFIX.2.fa PREFIX.s.fa (FASTQ input allowed)\n"
        "  --rule correct [--min-cover C]   with --extract FILE: every read whole, \">read_index n_corrected\", its isolated substitutions repaired; the counters go to stderr\n"
        "  --rule split   with --extract FILE: every run of k-mers with count >= N (--solid) as a record of its own, \">read_index start len\"; the counters go to stderr\n"
        "  --degrees FILE   the index as a de Bruijn graph: the 5 x 5 matrix of (left, right) degrees of the nodes (count >= --min-count) and a line \"below\" as TSV, the figures on stderr; k > 32 wants --full-minimizers\n"
        "  --prune-degrees L:R[,L:R...]   remove the nodes (--min-count <= count <= --max-count) with L left and R right neighbours, e.g. 0:0 the isolated ones; prints how many went\n"
        "  --saturate   counts stop at 255 (\"255 or more\") instead of wrapping at 256; snapshots carry the mode, and --histo labels its last line 255+\n"
        "  --full-minimizers   the minimizer re-scan sees the whole k-mer at k > 32 too (minimizer_mode full): one canonical k-mer, one entry; snapshots carry the mode";
    for (int i = 0; i < argc_in; i++) {
        if (i > 0 && (!strcmp(argv_in[i], "--help") || !strcmp(argv_in[i], "-h"))) {
            std::cout << usage << std::endl;
            return 0;
        }
        if (i > 0 && !strcmp(argv_in[i], "--saturate")) {
            saturate = true;
            continue;
        }
        if (i > 0 && !strcmp(argv_in[i], "--full-minimizers")) {
            full_minimizers = true;
            continue;
        }
        if (i > 0 && !strcmp(argv_in[i], "--paired")) {
            paired = true;
            continue;
        }
        int setop = -1;
        for (int q = 0; q < 3; q++)
            if (i > 0 && !strcmp(argv_in[i], setop_names[q])) setop = q;
        const bool named = i > 0 && (setop >= 0 || !strcmp(argv_in[i], "--histo") || !strcmp(argv_in[i], "--degrees") || !strcmp(argv_in[i], "--prune-degrees") || !strcmp(argv_in[i], "--save") || !strcmp(argv_in[i], "--load") || !strcmp(argv_in[i], "--min-count") || !strcmp(argv_in[i], "--max-count") ||
                                    !strcmp(argv_in[i], "--profile") || !strcmp(argv_in[i], "--solid") || !strcmp(argv_in[i], "--extract") || !strcmp(argv_in[i], "--rule") ||
                                    !strcmp(argv_in[i], "--min-len") || !strcmp(argv_in[i], "--min-cover") || !strcmp(argv_in[i], "--joint") || !strcmp(argv_in[i], "--joint-histo") || !strcmp(argv_in[i], "--filter-joint") ||
                                    !strcmp(argv_in[i], "--window") || !strcmp(argv_in[i], "--min-qual") || !strcmp(argv_in[i], "--qual-base") || !strcmp(argv_in[i], "--mate") ||
                                    !strcmp(argv_in[i], "--pair-mode"));
        if (!named) {
            args.push_back(argv_in[i]);
            continue;
        }
        if (i + 1 >= argc_in) {
            std::cerr << argv_in[i] << " needs a value" << std::endl;
            return 2;
        }
        const char* opt = argv_in[i++];
        if (!strcmp(opt, "--histo")) histo = argv_in[i];
        else if (!strcmp(opt, "--degrees")) degrees_file = argv_in[i];
        else if (!strcmp(opt, "--prune-degrees")) {
            prune_degrees_text = argv_in[i];
            for (const char* q = prune_degrees_text;;) {  // L:R[,L:R...], a degree is 0..4
                if (q[0] < '0' || q[0] > '4' || q[1] != ':' || q[2] < '0' || q[2] > '4' || (q[3] && q[3] != ',')) {
                    std::cerr << "--prune-degrees: L:R[,L:R...] with L and R in 0..4, got " << prune_degrees_text << std::endl;
                    return 2;
                }
                degree_mask |= 1u << (5 * (q[0] - '0') + (q[2] - '0'));
                if (!q[3]) break;
                q += 4;
            }
        }
        else if (!strcmp(opt, "--save")) save_file = argv_in[i];
        else if (!strcmp(opt, "--load")) load_file = argv_in[i];
        else if (!strcmp(opt, "--profile")) profile_file = argv_in[i];
        else if (!strcmp(opt, "--extract")) extract_file = argv_in[i];
        else if (!strcmp(opt, "--rule")) rule_text = argv_in[i];
        else if (!strcmp(opt, "--joint")) joint_file = argv_in[i];
        else if (!strcmp(opt, "--joint-histo")) joint_histo = argv_in[i];
        else if (!strcmp(opt, "--filter-joint")) filter_joint_file = argv_in[i];
        else if (!strcmp(opt, "--window")) window_text = argv_in[i];
        else if (!strcmp(opt, "--mate")) mate_file = argv_in[i];
        else if (!strcmp(opt, "--pair-mode")) pair_mode_text = argv_in[i];
        else if (!strcmp(opt, "--min-qual") || !strcmp(opt, "--qual-base")) {
            char* end = nullptr;
            const long v = strtol(argv_in[i], &end, 10);
            const bool mq = !strcmp(opt, "--min-qual");
            if (end == argv_in[i] || *end || (mq ? (v < 0 || v > 93) : (v != 33 && v != 64))) {
                std::cerr << opt << (mq ? ": a quality is 0..93, got " : ": 33 or 64, got ") << argv_in[i] << std::endl;
                return 2;
            }
            (mq ? min_qual : qual_base) = v;
            have_qual = true;
        }
        else if (!strcmp(opt, "--min-len")) {
            char* end = nullptr;
            min_len = strtol(argv_in[i], &end, 10);
            if (end == argv_in[i] || *end || min_len < 0 || min_len > 0xffffffffl) {
                std::cerr << "--min-len: a number of nucleotides, got " << argv_in[i] << std::endl;
                return 2;
            }
        }
        else if (!strcmp(opt, "--min-cover")) {
            char* end = nullptr;
            min_cover = strtol(argv_in[i], &end, 10);
            if (end == argv_in[i] || *end || min_cover < 0 || min_cover > 0xffffffffl) {
                std::cerr << "--min-cover: a number of k-mers, got " << argv_in[i] << std::endl;
                return 2;
            }
        }
        else if (!strcmp(opt, "--solid")) {  // (above 255: no k-mer is solid)
            char* end = nullptr;
            solid = strtol(argv_in[i], &end, 10);
            if (end == argv_in[i] || *end || solid < 0 || solid > 0xffffffffl) {
                std::cerr << "--solid: a count threshold, got " << argv_in[i] << std::endl;
                return 2;
            }
            have_solid = true;
        }
        else if (setop >= 0) {
            if (setop_file[setop]) {
                std::cerr << opt << " may be given once" << std::endl;
                return 2;
            }
            setop_file[setop] = argv_in[i];
        } else {
            char* end = nullptr;
            const long v = strtol(argv_in[i], &end, 10);
            if (end == argv_in[i] || *end || v < 0 || v > 255) {
                std::cerr << opt << ": a count is 0..255, got " << argv_in[i] << std::endl;
                return 2;
            }
            (!strcmp(opt, "--min-count") ? min_count : max_count) = v;
            have_range = true;
        }
    }
    const int argc = (int)args.size();
    char** argv = args.data();
    const bool have_setop = setop_file[0] || setop_file[1] || setop_file[2];
    if ((histo || degrees_file || prune_degrees_text || have_range || have_setop || joint_file || joint_histo || filter_joint_file || window_text || save_file || load_file || profile_file || have_solid || saturate || full_minimizers || extract_file || rule_text || min_len || have_qual || paired || mate_file || pair_mode_text) && (argc < 2 || strcmp(argv[1], "--bulk"))) {
        std::cerr << "--saturate, --full-minimizers, --histo, --degrees, --prune-degrees, --min-count, --max-count, --merge, --subtract, --intersect, --filter-joint, --window, --joint, --joint-histo, --save, --load, --profile, --solid, --extract, --rule, --min-len, --min-qual, --qual-base, --paired, --mate and --pair-mode work on the device "
                     "index: --bulk only" << std::endl;
        return 2;
    }
    if (have_solid && !profile_file && !extract_file) {
        std::cerr << "--solid is the threshold of --profile FILE and of --extract FILE" << std::endl;
        return 2;
    }
    if ((rule_text || min_len) && !extract_file) {
        std::cerr << "--rule and --min-len belong to --extract FILE" << std::endl;
        return 2;
    }
    if ((mate_file || pair_mode_text) && !paired) {
        std::cerr << "--mate FILE and --pair-mode belong to --paired" << std::endl;
        return 2;
    }
    if (min_cover >= 0 && !(extract_file && rule_text && !strcmp(rule_text, "correct"))) {
        std::cerr << "--min-cover belongs to --extract FILE --rule correct" << std::endl;
        return 2;
    }
    uint32_t pair_mode = BRISK_HIP_PAIR_EACH;
    if (pair_mode_text) {
        if (!strcmp(pair_mode_text, "each")) pair_mode = BRISK_HIP_PAIR_EACH;
        else if (!strcmp(pair_mode_text, "all")) pair_mode = BRISK_HIP_PAIR_ALL;
        else if (!strcmp(pair_mode_text, "any")) pair_mode = BRISK_HIP_PAIR_ANY;
        else {
            std::cerr << "--pair-mode: each, all or any, got " << pair_mode_text << std::endl;
            return 2;
        }
    }
    if (!joint_file != !joint_histo) {
        std::cerr << "--joint FILE and --joint-histo OUT come together" << std::endl;
        return 2;
    }
    if (!filter_joint_file != !window_text) {
        std::cerr << "--filter-joint FILE and --window SLO:SHI:OLO:OHI[:absent] come together" << std::endl;
        return 2;
    }
    brisk_hip_joint_window window{};
    if (window_text) {  // SLO:SHI:OLO:OHI or SLO:SHI:OLO:OHI:absent
        unsigned long v[4] = {0, 0, 0, 0};
        int used = 0;
        const bool four = sscanf(window_text, "%lu:%lu:%lu:%lu%n", &v[0], &v[1], &v[2], &v[3], &used) == 4;
        const char* tail = four ? window_text + used : "?";
        const bool digits_only = strspn(window_text, "0123456789:") >= (size_t)used;  // (no sign, no blank: sscanf would take them)
        if (!four || !digits_only || (*tail && strcmp(tail, ":absent")) || std::max(std::max(v[0], v[1]), std::max(v[2], v[3])) > 255 || v[0] > v[1] || (v[2] > v[3] && !*tail)) {
            std::cerr << "--window: SLO:SHI:OLO:OHI[:absent] with counts 0..255, SLO <= SHI, and OLO <= OHI unless :absent is given; got " << window_text << std::endl;
            return 2;
        }
        window.min_self = (uint32_t)v[0];
        window.max_self = (uint32_t)v[1];
        window.min_other = (uint32_t)v[2];
        window.max_other = (uint32_t)v[3];
        window.keep_absent = *tail ? 1 : 0;
    }
    brisk_hip_select_rule rule{};
    rule.struct_size = sizeof rule;
    rule.kind = BRISK_HIP_SELECT_SOLID_RUN;
    rule.min_len = (uint32_t)min_len;
    rule.hi = 0xffffffffu;
    const bool rule_split = rule_text && !strcmp(rule_text, "split");  // every solid run of a read, not one interval: brisk_hip_split_reads
    const bool rule_correct = rule_text && !strcmp(rule_text, "correct");  // every read whole, its isolated substitutions repaired: brisk_hip_correct_reads
    if (rule_text && strcmp(rule_text, "trim") && !rule_split && !rule_correct) {  // median:LO:HI or present:LO:HI
        unsigned long lo = 0, hi = 0;
        char tail = 0;
        if (sscanf(rule_text, "median:%lu:%lu%c", &lo, &hi, &tail) == 2) rule.kind = BRISK_HIP_SELECT_MEDIAN;
        else if (sscanf(rule_text, "present:%lu:%lu%c", &lo, &hi, &tail) == 2) rule.kind = BRISK_HIP_SELECT_PRESENT;
        else {
            std::cerr << "--rule: trim, median:LO:HI or present:LO:HI, got " << rule_text << std::endl;
            return 2;
        }
        if (lo > hi || hi > 0xfffffffful) {
            std::cerr << "--rule " << rule_text << ": LO <= HI < 2^32" << std::endl;
            return 2;
        }
        rule.lo = (uint32_t)lo;
        rule.hi = (uint32_t)hi;
    }
    if (min_count > max_count) {
        std::cerr << "--min-count " << min_count << " is above --max-count " << max_count << std::endl;
        return 2;
    }
    if (argc < 6) {
        std::cerr << usage << std::endl;
        return 2;
    }
    const bool bulk = !strcmp(argv[1], "--bulk");
    const size_t batch_bases = getenv("BRISK_BATCH_BASES") ? (size_t)atoll(getenv("BRISK_BATCH_BASES")) : ((size_t)256 << 20);
    const bool mixed = !strcmp(argv[1], "--mixed");
    const std::vector<std::string> seqs = (bulk || mixed) ? std::vector<std::string>() : read_fasta(argv[2]);
    const uint8_t k = (uint8_t)atoi(argv[3]), m = (uint8_t)atoi(argv[4]), b = (uint8_t)atoi(argv[5]);
    const char* dump = argc > 6 && strcmp(argv[6], "-") ? argv[6] : nullptr;
    const char* kff = argc > 7 ? argv[7] : nullptr;
    Parameters params(k, m, b);
    brisk_hip_intake_rule intake{};
    intake.struct_size = sizeof intake;
    intake.min_qual = (uint32_t)min_qual;
    intake.qual_base = (uint32_t)qual_base;
    const bool fastq_main = bulk && is_fastq(argv[2]);
    if (bulk && have_qual) {
        bool any = fastq_main;
        for (const char* f : {setop_file[0], setop_file[1], setop_file[2], filter_joint_file, joint_file}) any = any || (f && is_fastq(f));
        if (!any) {
            std::cerr << "--min-qual and --qual-base apply to FASTQ input, and no input is FASTQ" << std::endl;
            return 2;
        }
    }
    if (fastq_main && (profile_file || (extract_file && !paired))) {
        std::cerr << (profile_file ? "--profile" : "--extract") << " reads the input again as FASTA: not with a FASTQ input" << std::endl;
        return 2;
    }
    if (rule_split && paired) {
        std::cerr << "--rule split cuts reads into several fragments: not with --paired" << std::endl;
        return 2;
    }
    if (rule_correct && paired) {
        std::cerr << "--rule correct writes every read as one record of one file: not with --paired (correct the interleaved file, the records stay in step)" << std::endl;
        return 2;
    }
    if (paired) {  // whole pairs, before anything is counted
        if (!bulk || !strcmp(argv[2], "-") || is_snapshot(argv[2])) {
            std::cerr << "--paired needs reads: a FASTA or FASTQ input" << std::endl;
            return 2;
        }
        try {
            if (mate_file && (is_snapshot(mate_file) || is_fastq(mate_file) != fastq_main)) {
                std::cerr << "--mate " << mate_file << ": the two files of a paired input are both FASTA or both FASTQ" << std::endl;
                return 2;
            }
            uint64_t dirty1 = ~0ull, dirty2 = ~0ull;
            const uint64_t n1 = count_records(argv[2], fastq_main, &dirty1), n2 = mate_file ? count_records(mate_file, fastq_main, &dirty2) : 0;
            if (mate_file ? n1 != n2 : n1 % 2 != 0) {
                if (mate_file) std::cerr << "--paired: " << argv[2] << " holds " << n1 << " reads, --mate " << mate_file << " " << n2 << std::endl;
                else std::cerr << "--paired: " << argv[2] << " holds " << n1 << " reads, an odd number: an interleaved file holds whole pairs" << std::endl;
                return 2;
            }
            if (dirty1 != ~0ull || dirty2 != ~0ull) {  // (FASTA only; in two files the earlier pair is named)
                const bool second = mate_file ? dirty2 < dirty1 : (dirty1 & 1) != 0;
                const uint64_t pair = mate_file ? std::min(dirty1, dirty2) : dirty1 / 2;
                std::cerr << "--paired: mate " << (second ? 2 : 1) << " of pair " << pair << " holds a byte that is no base: paired FASTA records must be clean (FASTQ input is cut on the device)" << std::endl;
                return 2;
            }
        } catch (const std::exception& e) {
            std::cerr << "--paired: " << e.what() << std::endl;
            return 1;
        }
    }
    if (mixed) return run_mixed(argv[2], k, m, b, params.dede->coef(), batch_bases);
    std::vector<std::string> lines;
    uint64_t nb_buckets = 0, nb_skmers = 0, nb_kmers = 0, mem = 0, largest = 0, sum = 0;
    try {
        if (!bulk) {
            Brisk<uint8_t> index(params);
            for (const std::string& s0 : seqs) {
                if (s0.size() < k) continue;
                std::string s(s0);
                SuperKmerEnumerator en(s, k, m, params.dede);
                std::vector<kmer_full> v;
                std::vector<bool> fresh;
                en.next(v);
                while (!v.empty()) {
                    fresh.clear();
                    index.protect_data(v[0]);
                    std::vector<uint8_t*> ptr = index.insert_superkmer(v, fresh);
                    for (size_t i = 0; i < ptr.size(); i++) {
                        if (fresh[i]) *ptr[i] = 1;
                        else ++*ptr[i];
                    }
                    index.unprotect_data(v[0]);
                    v.clear();
                    en.next(v);
                }
            }
            if (getenv("BRISK_REALLOCATE")) {  // Brisk::reallocate (brisk/Brisk.hpp:202-224): the same entries under (k, m + 2, b + 2)
                index.reallocate();
                std::cout << "reallocated k " << (int)index.params.k << " m " << (int)index.params.m << " b " << (int)index.params.b << std::endl;
            }
            kmer_full km((kint)0, 0, index.params.m, index.params.dede);
            bool first_entry = true;
            while (index.next(km)) {
                uint8_t* c = index.get(km);
                if (!c) {
                    std::cerr << "entry without data" << std::endl;
                    return 1;
                }
                if (first_entry) {  // Brisk::insert on a k-mer that is present behaves like get (README.md:49 of the reference)
                    first_entry = false;
                    if (index.insert(km) != c) {
                        std::cerr << "insert(kmer) of a present k-mer is not its get" << std::endl;
                        return 1;
                    }
                }
                sum += *c;
                if (dump) lines.push_back(kmer2str(km.kmer_s, k) + " " + std::to_string(km.minimizer_idx) + " " + std::to_string(*c));
            }
            index.stats(nb_buckets, nb_skmers, nb_kmers, mem, largest);
            if (kff) {  // apps/counter.cpp:407-411
                BriskWriter writer(kff);
                writer.write(index);
                writer.close();
            }
        } else {
            brisk_hip_options o{};
            o.struct_size = sizeof o;
            o.count_mode = saturate ? BRISK_HIP_COUNTS_SATURATE : BRISK_HIP_COUNTS_WRAP;  // (also the second index's of a set operation)
            o.minimizer_mode = full_minimizers ? BRISK_HIP_MINIMIZER_FULL : BRISK_HIP_MINIMIZER_REFERENCE;
            brisk_hip_index* h = nullptr;
            int rc = brisk_hip_create(&h, k, m, b, 1, params.dede->coef(), &o);
            if (rc != BRISK_HIP_OK) {
                std::cerr << "brisk_hip_create failed: " << rc << std::endl;
                return 1;
            }
            // stream the file: a background thread inflates and segments batch i+1 while the GPU counts batch i
            const bool e2e = getenv("BRISK_E2E_JSON") != nullptr;  // bench.py's end-to-end leg: the stage split as one JSON line
            if (e2e) brisk_hip_profile_enable(h, 1);
            if (load_file) {  // start from the snapshot; slices with room, since the reads are counted on top
                if (int lrc = load_snapshot(h, "--load", load_file, k, m, b, BRISK_HIP_LOAD_ROOM)) return lrc;
            }
            const bool no_reads = !strcmp(argv[2], "-");
            const auto t_start = std::chrono::steady_clock::now();
            double insert_calls_s = 0.0;
            uint64_t n_reads_in = 0, n_bases_in = 0, n_batches = 0;
            if (no_reads) brisk_hip_stats(h, &nb_buckets, &nb_skmers, &nb_kmers, &mem, &largest);
            else if (fastq_main) {
                double produce_s = 0.0, wait_s = 0.0;
                if (count_fastq(h, argv[2], intake, batch_bases, &produce_s, &wait_s)) return 1;
                brisk_hip_sync(h);  // (completes deferred inserts: the index is whole when the clock stops)
                const double wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
                brisk_hip_stats(h, &nb_buckets, &nb_skmers, &nb_kmers, &mem, &largest);
                if (e2e)
                    std::cout << "E2E {\"wall_s\": " << wall_s << ", \"entries\": " << nb_kmers << ", \"reader_produce_s\": " << produce_s << ", \"main_waits_for_reader_s\": " << wait_s << "}"
                              << std::endl;
            } else {
                FastaBatcher batches(argv[2], batch_bases);
                FastaBatch bt;
                while (batches.next(bt)) {
                    const auto c0 = std::chrono::steady_clock::now();
                    rc = brisk_hip_insert_reads(h, bt.flat.data(), bt.offs.data(), bt.size());
                    insert_calls_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
                    if (rc != BRISK_HIP_OK) {
                        std::cerr << brisk_hip_last_error(h) << std::endl;
                        return 1;
                    }
                    n_reads_in += bt.size();
                    n_bases_in += bt.flat.size();
                    n_batches++;
                }
                const auto c0 = std::chrono::steady_clock::now();
                brisk_hip_sync(h);  // (completes deferred inserts: the index is whole when the clock stops)
                const double sync_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
                const double wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
                brisk_hip_stats(h, &nb_buckets, &nb_skmers, &nb_kmers, &mem, &largest);
                if (e2e) {
                    uint32_t ns = 0;
                    const char* names[BRISK_HIP_PROFILE_SLOTS];
                    uint64_t launches[BRISK_HIP_PROFILE_SLOTS];
                    double ms[BRISK_HIP_PROFILE_SLOTS];
                    brisk_hip_profile_read(h, &ns, names, launches, ms);
                    std::cout << "E2E {\"wall_s\": " << wall_s << ", \"reads\": " << n_reads_in << ", \"bases\": " << n_bases_in << ", \"batches\": " << n_batches
                              << ", \"entries\": " << nb_kmers << ", \"reader_produce_s\": " << batches.produce_seconds() << ", \"main_waits_for_reader_s\": "
                              << batches.consumer_wait_seconds() << ", \"insert_reads_calls_s\": " << insert_calls_s << ", \"final_sync_s\": " << sync_s << ", \"library_ms\": {";
                    bool first = true;
                    for (uint32_t i = 0; i < ns; i++)
                        if (launches[i]) {
                            std::cout << (first ? "" : ", ") << "\"" << names[i] << "\": " << ms[i];
                            first = false;
                        }
                    std::cout << "}}" << std::endl;
                }
            }
            if (mate_file) {  // the mates' file is counted like the input: pairing never changes the index
                if (fastq_main) {
                    if (count_fastq(h, mate_file, intake, batch_bases)) return 1;
                } else {
                    FastaBatcher batches(mate_file, batch_bases);
                    FastaBatch bt;
                    while (batches.next(bt))
                        if (brisk_hip_insert_reads(h, bt.flat.data(), bt.offs.data(), bt.size()) != BRISK_HIP_OK) {
                            std::cerr << "--mate: " << brisk_hip_last_error(h) << std::endl;
                            return 1;
                        }
                }
                brisk_hip_sync(h);
                brisk_hip_stats(h, &nb_buckets, &nb_skmers, &nb_kmers, &mem, &largest);
            }
            // FILE of a set operation counted (or, a snapshot, loaded) into a second index of the same parameters; 0 or the exit status
            auto second_index = [&](const char* opt, const char* file, brisk_hip_index** out) -> int {
                brisk_hip_index* other = nullptr;
                const int crc = brisk_hip_create(&other, k, m, b, 1, params.dede->coef(), &o);
                if (crc != BRISK_HIP_OK) {
                    std::cerr << opt << ": brisk_hip_create failed: " << crc << std::endl;
                    return 1;
                }
                if (is_snapshot(file)) {  // the second index from its snapshot: compact, it only serves this operation
                    if (int lrc = load_snapshot(other, opt, file, k, m, b, BRISK_HIP_LOAD_COMPACT)) return lrc;
                } else if (is_fastq(file)) {
                    if (count_fastq(other, file, intake, batch_bases)) return 1;
                } else {
                    FastaBatcher batches(file, batch_bases);
                    FastaBatch bt;
                    while (batches.next(bt))
                        if (brisk_hip_insert_reads(other, bt.flat.data(), bt.offs.data(), bt.size()) != BRISK_HIP_OK) {
                            std::cerr << opt << ": " << brisk_hip_last_error(other) << std::endl;
                            return 1;
                        }
                }
                *out = other;
                return 0;
            };
            for (int q = 0; q < 3; q++) {  // --merge, --subtract, --intersect: FILE counted into a second index, then combined on the device
                if (!setop_file[q]) continue;
                brisk_hip_index* other = nullptr;
                if (int src = second_index(setop_names[q], setop_file[q], &other)) return src;
                uint64_t changed = 0;
                rc = q == 0 ? brisk_hip_merge(h, other, &changed) : q == 1 ? brisk_hip_subtract(h, other, &changed) : brisk_hip_intersect(h, other, BRISK_HIP_COUNT_LEFT, &changed);
                if (rc != BRISK_HIP_OK) {
                    std::cerr << setop_names[q] << ": " << brisk_hip_last_error(h) << std::endl;
                    return 1;
                }
                std::cerr << (setop_names[q] + 2) << " " << setop_file[q] << ": " << changed << (q == 0 ? " entries added" : " entries removed") << std::endl;
                brisk_hip_destroy(other);
                brisk_hip_stats(h, &nb_buckets, &nb_skmers, &nb_kmers, &mem, &largest);
            }
            if (filter_joint_file) {
                brisk_hip_index* other = nullptr;
                if (int src = second_index("--filter-joint", filter_joint_file, &other)) return src;
                uint64_t gone = 0;
                if (brisk_hip_filter_joint(h, other, &window, &gone) != BRISK_HIP_OK) {
                    std::cerr << "--filter-joint: " << brisk_hip_last_error(h) << std::endl;
                    return 1;
                }
                std::cerr << "filter-joint " << filter_joint_file << " " << window_text << ": " << gone << " entries removed" << std::endl;
                brisk_hip_destroy(other);
                brisk_hip_stats(h, &nb_buckets, &nb_skmers, &nb_kmers, &mem, &largest);
            }
            if ((save_file || profile_file || extract_file || joint_file) && have_range) {  // the final index: what the dump below shows is what the file holds and what the reads are profiled against
                uint64_t gone = 0;
                if (brisk_hip_prune(h, (uint32_t)min_count, (uint32_t)max_count, &gone) != BRISK_HIP_OK) {
                    std::cerr << (save_file ? "--save" : profile_file ? "--profile" : extract_file ? "--extract" : "--joint") << ": prune: " << brisk_hip_last_error(h) << std::endl;
                    return 1;
                }
                brisk_hip_stats(h, &nb_buckets, &nb_skmers, &nb_kmers, &mem, &largest);
            }
            if (joint_file) {  // the final index against FILE's: one line per non-zero bin, absent (-1) last on both axes
                brisk_hip_index* other = nullptr;
                if (int src = second_index("--joint", joint_file, &other)) return src;
                std::vector<uint64_t> joint((size_t)BRISK_HIP_JOINT_STATES * BRISK_HIP_JOINT_STATES);
                if (brisk_hip_joint_spectrum(h, other, joint.data()) != BRISK_HIP_OK) {
                    std::cerr << "--joint: " << brisk_hip_last_error(h) << std::endl;
                    return 1;
                }
                brisk_hip_destroy(other);
                std::ofstream out(joint_histo);
                uint64_t bins = 0;
                for (uint32_t sa = 0; sa < BRISK_HIP_JOINT_STATES; sa++)
                    for (uint32_t sb = 0; sb < BRISK_HIP_JOINT_STATES; sb++) {
                        const uint64_t n = joint[(size_t)sa * BRISK_HIP_JOINT_STATES + sb];
                        if (!n) continue;
                        out << (sa == BRISK_HIP_JOINT_ABSENT ? -1 : (int)sa) << "\t" << (sb == BRISK_HIP_JOINT_ABSENT ? -1 : (int)sb) << "\t" << n << "\n";
                        bins++;
                    }
                out.close();
                if (!out) {
                    std::cerr << "--joint-histo " << joint_histo << ": write failed" << std::endl;
                    return 1;
                }
                std::cerr << "joint " << joint_file << ": " << bins << " non-zero bins" << std::endl;
            }
            if (save_file) {
                uint64_t written = 0;
                if (brisk_hip_save(h, save_file, &written) != BRISK_HIP_OK) {
                    std::cerr << "--save " << save_file << ": " << brisk_hip_last_error(h) << std::endl;
                    return 1;
                }
                std::cerr << "save " << save_file << ": " << written << " entries written" << std::endl;
            }
            if (profile_file) {  // the reads of the input again, in input order, against the final index: one line per read
                std::ofstream out(profile_file);
                out << "#read_index\tn_kmers\tn_present\tn_solid\trun_start\trun_len\tmin\tmax\tmedian\tmedian_present\tsum\n";
                uint64_t read_index = 0;
                if (!no_reads) {
                    FastaBatcher batches(argv[2], batch_bases);
                    FastaBatch bt;
                    std::vector<brisk_hip_read_profile> recs;
                    while (batches.next(bt)) {
                        recs.resize(bt.size());
                        if (brisk_hip_read_profile_reads(h, bt.flat.data(), bt.offs.data(), bt.size(), (uint32_t)solid, recs.data()) != BRISK_HIP_OK) {
                            std::cerr << "--profile: " << brisk_hip_last_error(h) << std::endl;
                            return 1;
                        }
                        for (const brisk_hip_read_profile& r : recs)
                            out << read_index++ << "\t" << r.n_kmers << "\t" << r.n_present << "\t" << r.n_solid << "\t" << r.run_start << "\t" << r.run_len << "\t" << (unsigned)r.min_present
                                << "\t" << (unsigned)r.max_present << "\t" << (unsigned)r.median << "\t" << (unsigned)r.median_present << "\t" << r.sum << "\n";
                    }
                }
                out.close();
                if (!out) {
                    std::cerr << "--profile " << profile_file << ": write failed" << std::endl;
                    return 1;
                }
                std::cerr << "profile " << profile_file << ": " << read_index << " reads, solid >= " << solid << std::endl;
            }
            if (extract_file && paired) {
                if (int erc = extract_paired(h, argv[2], mate_file, fastq_main, extract_file, rule, (uint32_t)solid, intake, pair_mode, batch_bases)) return erc;
            } else if (extract_file && rule_split) {  // the reads of the input again, against the final index: one record per fragment, in table order
                std::ofstream out(extract_file);
                brisk_hip_split_stats sum{};
                uint64_t read_index = 0;
                if (!no_reads) {
                    FastaBatcher batches(argv[2], batch_bases);
                    FastaBatch bt;
                    std::vector<brisk_hip_fragment> frags;
                    while (batches.next(bt)) {
                        brisk_hip_split_stats st{};
                        int src = brisk_hip_split_reads(h, bt.flat.data(), bt.offs.data(), bt.size(), (uint32_t)solid, (uint32_t)min_len, frags.data(), frags.size(), &st);
                        if (src == BRISK_HIP_ECAPACITY) {  // (the refused call has counted them)
                            frags.resize(st.n_fragments);
                            src = brisk_hip_split_reads(h, bt.flat.data(), bt.offs.data(), bt.size(), (uint32_t)solid, (uint32_t)min_len, frags.data(), frags.size(), &st);
                        }
                        if (src != BRISK_HIP_OK) {
                            std::cerr << "--extract: " << brisk_hip_last_error(h) << std::endl;
                            return 1;
                        }
                        for (uint64_t j = 0; j < st.n_fragments; j++) {
                            const brisk_hip_fragment& f = frags[j];
                            out << ">" << read_index + f.read << " " << f.start << " " << f.len << "\n";
                            out.write(bt.flat.data() + bt.offs[f.read] + f.start, f.len);
                            out << "\n";
                        }
                        read_index += bt.size();
                        const uint64_t* add = (const uint64_t*)&st;
                        for (size_t i = 0; i < sizeof(st) / 8; i++) ((uint64_t*)&sum)[i] += add[i];
                    }
                }
                out.close();
                if (!out) {
                    std::cerr << "--extract " << extract_file << ": write failed" << std::endl;
                    return 1;
                }
                std::cerr << "extract " << extract_file << ": " << sum.n_fragments << " fragments of " << sum.n_reads_kept << " of " << sum.n_reads << " reads, " << sum.n_nts_out << " of "
                          << sum.n_nts_in << " nucleotides, " << sum.n_solid << " of " << sum.n_slots << " k-mers solid, " << sum.n_short << " in short runs (--rule split, solid >= "
                          << solid << ")" << std::endl;
            } else if (extract_file && rule_correct) {  // the reads of the input again, against the final index: every read, repaired, one record each
                std::ofstream out(extract_file);
                brisk_hip_correct_stats sum{};
                uint64_t read_index = 0, reads_changed = 0;
                const uint32_t cover = min_cover < 0 ? 0u : (uint32_t)min_cover;
                if (!no_reads) {
                    FastaBatcher batches(argv[2], batch_bases);
                    FastaBatch bt;
                    std::vector<brisk_hip_correction> corr;
                    std::string seq;
                    while (batches.next(bt)) {
                        brisk_hip_correct_stats st{};
                        int crc = brisk_hip_correct_reads(h, bt.flat.data(), bt.offs.data(), bt.size(), (uint32_t)solid, cover, corr.data(), corr.size(), &st);
                        if (crc == BRISK_HIP_ECAPACITY) {  // (the refused call has counted them)
                            corr.resize(st.n_corrected);
                            crc = brisk_hip_correct_reads(h, bt.flat.data(), bt.offs.data(), bt.size(), (uint32_t)solid, cover, corr.data(), corr.size(), &st);
                        }
                        if (crc != BRISK_HIP_OK) {
                            std::cerr << "--extract: " << brisk_hip_last_error(h) << std::endl;
                            return 1;
                        }
                        uint64_t j = 0;  // the table is ordered by read, then by position
                        for (uint64_t r = 0; r < bt.size(); r++) {
                            seq.assign(bt.flat.data() + bt.offs[r], bt.offs[r + 1] - bt.offs[r]);
                            uint64_t n = 0;
                            for (; j < st.n_corrected && corr[j].read == r; j++, n++) seq[corr[j].pos] = "ACTG"[corr[j].to & 3];
                            reads_changed += n > 0;
                            out << ">" << read_index + r << " " << n << "\n" << seq << "\n";
                        }
                        read_index += bt.size();
                        const uint64_t* add = (const uint64_t*)&st;
                        for (size_t i = 0; i < sizeof(st) / 8; i++) ((uint64_t*)&sum)[i] += add[i];
                    }
                }
                out.close();
                if (!out) {
                    std::cerr << "--extract " << extract_file << ": write failed" << std::endl;
                    return 1;
                }
                std::cerr << "extract " << extract_file << ": " << sum.n_corrected << " corrections in " << reads_changed << " of " << sum.n_reads << " reads, " << sum.n_sites << " sites ("
                          << sum.n_ambiguous << " ambiguous, " << sum.n_unresolved << " unresolved) of " << sum.n_runs << " weak runs (" << sum.n_skip_whole << " whole, " << sum.n_skip_long
                          << " long, " << sum.n_skip_short << " short), " << sum.n_weak << " of " << sum.n_slots << " k-mers weak (--rule correct, solid >= " << solid << ", min-cover "
                          << cover << ")" << std::endl;
            } else if (extract_file) {  // the reads of the input again, against the final index: what the rule keeps of them, as FASTA
                std::ofstream out(extract_file);
                uint64_t read_index = 0, kept = 0, kept_nts = 0;
                if (!no_reads) {
                    FastaBatcher batches(argv[2], batch_bases);
                    FastaBatch bt;
                    std::vector<brisk_hip_read_interval> ivs;
                    while (batches.next(bt)) {
                        ivs.resize(bt.size());
                        if (brisk_hip_trim_reads(h, bt.flat.data(), bt.offs.data(), bt.size(), (uint32_t)solid, &rule, ivs.data()) != BRISK_HIP_OK) {
                            std::cerr << "--extract: " << brisk_hip_last_error(h) << std::endl;
                            return 1;
                        }
                        for (size_t i = 0; i < bt.size(); i++, read_index++) {
                            if (!ivs[i].len) continue;
                            out << ">" << read_index << " " << ivs[i].start << " " << ivs[i].len << "\n";
                            out.write(bt.flat.data() + bt.offs[i] + ivs[i].start, ivs[i].len);
                            out << "\n";
                            kept++;
                            kept_nts += ivs[i].len;
                        }
                    }
                }
                out.close();
                if (!out) {
                    std::cerr << "--extract " << extract_file << ": write failed" << std::endl;
                    return 1;
                }
                std::cerr << "extract " << extract_file << ": " << kept << " of " << read_index << " reads, " << kept_nts << " nucleotides (--rule " << (rule_text ? rule_text : "trim")
                          << ")" << std::endl;
            }
            if (histo) {
                uint64_t spectrum[256];
                if (brisk_hip_count_spectrum(h, spectrum) != BRISK_HIP_OK) {
                    std::cerr << "histo: " << brisk_hip_last_error(h) << std::endl;
                    return 1;
                }
                std::ofstream out(histo);
                // a saturating index: no count wrapped, and the last bin holds everything seen 255 times or more
                if (saturate) out << "# counts saturate (--saturate): the last line, 255+, is the entries seen 255 times or more\n";
                for (int c = 0; c < 255; c++) out << c << "\t" << spectrum[c] << "\n";
                out << (saturate ? "255+" : "255") << "\t" << spectrum[255] << "\n";
            }
            if (degrees_file) {
                uint64_t sp[26];
                if (brisk_hip_degree_spectrum(h, (uint32_t)min_count, sp) != BRISK_HIP_OK) {
                    std::cerr << "--degrees: " << brisk_hip_last_error(h) << std::endl;
                    return 1;
                }
                std::ofstream out(degrees_file);
                uint64_t nodes = 0, ends = 0, dead = 0, branching = 0;
                for (int l = 0; l < 5; l++) {
                    for (int r = 0; r < 5; r++) {
                        const uint64_t v = sp[5 * l + r];
                        out << v << (r < 4 ? "\t" : "\n");
                        nodes += v;
                        ends += v * (uint64_t)(l + r);
                        if ((l == 0) != (r == 0)) dead += v;
                        if (l > 1 || r > 1) branching += v;
                    }
                }
                out << "below\t" << sp[25] << "\n";
                out.close();
                if (!out) {
                    std::cerr << "--degrees " << degrees_file << ": write failed" << std::endl;
                    return 1;
                }
                std::cerr << "degrees " << degrees_file << ": " << nodes << " nodes, " << ends << " edge ends, " << sp[0] << " isolated, " << dead << " dead ends, " << sp[6] << " simple, "
                          << branching << " branching, " << sp[25] << " below --min-count" << std::endl;
            }
            if (prune_degrees_text) {
                uint64_t gone = 0;
                if (brisk_hip_prune_degrees(h, (uint32_t)min_count, (uint32_t)max_count, degree_mask, &gone) != BRISK_HIP_OK) {
                    std::cerr << "--prune-degrees: " << brisk_hip_last_error(h) << std::endl;
                    return 1;
                }
                std::cerr << "prune-degrees " << prune_degrees_text << ": " << gone << " entries removed" << std::endl;
                brisk_hip_stats(h, &nb_buckets, &nb_skmers, &nb_kmers, &mem, &largest);
            }
            uint64_t cursor = 0, n = 0;
            const uint64_t cap = 1u << 20;
            std::vector<uint64_t> lo(cap), hi(cap);
            std::vector<uint8_t> idx(cap), cnt(cap);
            for (;;) {
                rc = have_range ? brisk_hip_enumerate_range(h, &cursor, lo.data(), hi.data(), idx.data(), cnt.data(), cap, &n, (uint32_t)min_count, (uint32_t)max_count)
                                : brisk_hip_enumerate(h, &cursor, lo.data(), hi.data(), idx.data(), cnt.data(), cap, &n);
                if (rc != BRISK_HIP_OK || n == 0) break;
                for (uint64_t i = 0; i < n; i++) {
                    sum += cnt[i];
                    if (dump) lines.push_back(kmer2str(((kint)hi[i] << 64) | lo[i], k) + " " + std::to_string(idx[i]) + " " + std::to_string(cnt[i]));
                }
            }
            if (kff && brisk_write_kff(h, kff, (uint32_t)min_count, (uint32_t)max_count) != BRISK_HIP_OK) {
                std::cerr << "KFF: " << brisk_hip_last_error(h) << std::endl;
                return 1;
            }
            brisk_hip_destroy(h);
        }
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "nb_kmers " << nb_kmers << " nb_buckets " << nb_buckets << " sum_counts " << sum << std::endl;
    if (dump) {
        std::sort(lines.begin(), lines.end());
        std::ofstream out(dump);
        for (auto& l : lines) out << l << "\n";
    }
    return 0;
}
