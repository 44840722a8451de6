// prints every record the host FASTQ front-end yields for a FASTQ / FASTQ.gz file: "<bases>\t<qualities>" per line, and a
// "#batch N" line in front of every batch of N records; a malformed file: the message on stderr, exit status 1
#include <iostream>

#include "brisk_fastq.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    try {
        std::cout << "#first " << first_inflated_byte(argv[1]) << "\n";
        FastqBatcher batches(argv[1], (size_t)atoll(argv[2]));
        FastqBatch b;
        while (batches.next(b)) {
            std::cout << "#batch " << b.size() << "\n";
            for (size_t i = 0; i < b.size(); i++)
                std::cout << b.bases.substr(b.offs[i], b.offs[i + 1] - b.offs[i]) << "\t" << b.quals.substr(b.offs[i], b.offs[i + 1] - b.offs[i]) << "\n";
        }
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
