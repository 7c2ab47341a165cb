// Drives thermite::ThermiteAligner::align_read_records (include/thermite.hpp): the return shape of the reference's
// wrapper (src/wrapper.rs:64-101,126-141) -- BAM-encoded records without TX / GX / GN / RE -- one read per call.
//   bam_main <index file> <min_seed_len> <min_aln_score> <fastq> <out: stripped records> <out: records with tags>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "thermite.hpp"

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  try {
    thermite::ThermiteAligner a(argv[1]);
    a.opts_mut().min_seed_len = (std::size_t)atoi(argv[2]);
    a.opts_mut().min_aln_score = atoi(argv[3]);
    std::ifstream f(argv[4]);
    std::ofstream stripped(argv[5], std::ios::binary), tagged(argv[6], std::ios::binary);
    std::string name, seq, plus, qual;
    std::size_t n = 0;
    while (std::getline(f, name) && std::getline(f, seq) && std::getline(f, plus) && std::getline(f, qual)) {
      for (const auto& rec : a.align_read_records(name.substr(1), seq, qual)) {
        stripped.write(rec.data(), (std::streamsize)rec.size());
        n++;
      }
      for (const auto& rec : a.align_read_records_with_tags(name.substr(1), seq, qual)) tagged.write(rec.data(), (std::streamsize)rec.size());
    }
    fprintf(stderr, "records %zu\n", n);
  } catch (const thermite::Error& e) {
    fprintf(stderr, "error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
