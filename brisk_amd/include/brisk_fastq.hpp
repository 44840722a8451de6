// brisk_fastq.hpp -- host FASTQ / FASTQ.gz front-end for the raw intake (brisk_hip_insert_raw_reads).  No reference counterpart: the
// reference's harness reads FASTA only (apps/counter.cpp:130-190).
//   * strict four-line records: '@' header, ONE sequence line, '+' line, one quality line of the same length;
//   * a trailing '\r' is stripped from every line, and the last line may lack its newline;
//   * anything else throws, naming the record (counted from 1);
//   * nothing is cleaned: bases and qualities reach the device as read, where N and low quality are cut.
// Input is inflated with zlib (gzread reads plain files transparently).  FastqBatcher parses in the background, in one thread, while
// the GPU counts the previous batch: the shape of FastaBatcher.
#ifndef BRISK_AMD_FASTQ_HPP
#define BRISK_AMD_FASTQ_HPP
#include <zlib.h>

#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

struct FastqBatch {
    std::string bases, quals;    // concatenated sequence lines and quality lines: quals[i] belongs to bases[i]
    std::vector<uint64_t> offs;  // offs[n+1]: record r is [offs[r], offs[r + 1]) of both
    size_t size() const { return offs.empty() ? 0 : offs.size() - 1; }
    void clear() {
        bases.clear();
        quals.clear();
        offs.assign(1, 0);
    }
};

// the first inflated byte of a file ('@': FASTQ; '>' or anything else: not), -1 for an empty or unreadable file
inline int first_inflated_byte(const std::string& path) {
    gzFile gz = gzopen(path.c_str(), "rb");
    if (!gz) return -1;
    unsigned char c = 0;
    const int n = gzread(gz, &c, 1);
    gzclose(gz);
    return n == 1 ? (int)c : -1;
}

class FastqReader {
  public:
    explicit FastqReader(const std::string& path) : gz_(gzopen(path.c_str(), "rb")) {
        if (!gz_) throw std::runtime_error("cannot open " + path);
        gzbuffer(gz_, 1 << 20);
        buf_.resize(8 << 20);
    }
    ~FastqReader() {
        if (gz_) gzclose(gz_);
    }
    FastqReader(const FastqReader&) = delete;
    FastqReader& operator=(const FastqReader&) = delete;

    // Appends whole records to `out` until it holds at least max_bases bases or the file ends.  Returns false when nothing was
    // appended and the file is exhausted.
    bool fill(FastqBatch& out, size_t max_bases) {
        if (out.offs.empty()) out.offs.assign(1, 0);
        const size_t before = out.size();
        while (out.bases.size() < max_bases || out.size() == before) {
            if (!next_line(head_)) break;  // the end of the file, between two records
            n_rec_++;
            if (head_.empty() || head_[0] != '@') bad("the header line does not start with '@'");
            const size_t o = out.bases.size();
            if (!append_line(out.bases)) bad("the file ends after the header line");
            if (!next_line(plus_)) bad("the file ends after the sequence line");
            if (plus_.empty() || plus_[0] != '+') bad("the third line does not start with '+' (multi-line records are not supported)");
            if (!append_line(out.quals)) bad("the file ends after the '+' line");
            if (out.quals.size() != out.bases.size())
                bad("the quality line has " + std::to_string(out.quals.size() - o) + " characters, the sequence line " + std::to_string(out.bases.size() - o));
            out.offs.push_back(out.bases.size());
        }
        return out.size() > before;
    }
    bool done() const { return eof_ && pos_ == len_; }
    uint64_t records() const { return n_rec_; }

  private:
    [[noreturn]] void bad(const std::string& what) const { throw std::runtime_error("FASTQ record " + std::to_string(n_rec_) + ": " + what); }
    bool refill() {
        if (eof_) return false;
        const int n = gzread(gz_, &buf_[0], (unsigned)buf_.size());
        if (n < 0) throw std::runtime_error("gzread failed");
        pos_ = 0;
        len_ = (size_t)n;
        if (n == 0) eof_ = true;
        return n > 0;
    }
    // the next line, without its '\n' and without a '\r' before it, appended to `to`; false at the end of the file (nothing appended).
    // A last line without a newline counts when it holds anything.
    bool append_line(std::string& to) {
        const size_t o = to.size();
        bool any = false;
        for (;;) {
            if (pos_ == len_ && !refill()) break;
            any = true;
            const char* p = &buf_[pos_];
            const char* nl = (const char*)memchr(p, '\n', len_ - pos_);
            const size_t n = nl ? (size_t)(nl - p) : len_ - pos_;
            to.append(p, n);
            pos_ += n;
            if (nl) {
                pos_++;
                if (to.size() > o && to.back() == '\r') to.pop_back();
                return true;
            }
        }
        if (any && to.size() > o && to.back() == '\r') to.pop_back();
        return any;
    }
    bool next_line(std::string& line) {
        line.clear();
        return append_line(line);
    }
    gzFile gz_;
    std::string buf_, head_, plus_;
    size_t pos_ = 0, len_ = 0;
    bool eof_ = false;
    uint64_t n_rec_ = 0;
};

// Double-buffered batches: a background thread inflates and parses batch i+1 while the caller consumes batch i.
class FastqBatcher {
  public:
    FastqBatcher(const std::string& path, size_t batch_bases) : reader_(path), batch_bases_(batch_bases) {
        worker_ = std::thread([this] { run(); });
    }
    ~FastqBatcher() {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        if (worker_.joinable()) worker_.join();
    }
    // seconds the worker spent producing batches (inflate + parse), and seconds next() made its caller wait for a batch
    double produce_seconds() const { return produce_s_; }
    double consumer_wait_seconds() const { return wait_s_; }
    // Moves the next batch into `out`; false when the file is exhausted.  A malformed record throws here.
    bool next(FastqBatch& out) {
        const auto w0 = std::chrono::steady_clock::now();
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return ready_ || finished_; });
        wait_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
        if (!ready_) {
            if (!error_.empty()) throw std::runtime_error(error_);
            return false;
        }
        std::swap(out, slot_);
        ready_ = false;
        lk.unlock();
        cv_.notify_all();
        return true;
    }

  private:
    void run() {
        try {
            FastqBatch b;  // buffers circulate: what next() swapped back into the slot is filled again
            for (;;) {
                const auto p0 = std::chrono::steady_clock::now();
                b.clear();
                const bool more = reader_.fill(b, batch_bases_);
                produce_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - p0).count();
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this] { return !ready_ || stop_; });
                if (stop_) return;
                if (more) {
                    std::swap(slot_, b);
                    ready_ = true;
                } else {
                    finished_ = true;
                }
                lk.unlock();
                cv_.notify_all();
                if (!more) return;
            }
        } catch (const std::exception& e) {  // the batches before the bad record have been handed over; the error comes after them
            std::lock_guard<std::mutex> g(mu_);
            error_ = e.what();
            finished_ = true;
            cv_.notify_all();
        }
    }
    FastqReader reader_;
    size_t batch_bases_;
    FastqBatch slot_;
    double produce_s_ = 0.0, wait_s_ = 0.0;
    bool ready_ = false, finished_ = false, stop_ = false;
    std::string error_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::thread worker_;
};

#endif
