// Calls the per-hit methods of thermite::Aligner (include/thermite.hpp): extend_left_right and align_seed_hits
// (reference src/aligner.rs:352-407, 198-314).  Compiled by tests/test_seed_hits_host.py; it runs only where a GPU is
// visible (an aligner cannot be created without one).
//   seed_hits_main <index file>
#include <cstdio>
#include <string>
#include <vector>

#include "thermite.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  try {
    thermite::Index ix = thermite::Index::load(argv[1]);
    thermite::Aligner a(ix, thermite::AlignOpts());
    // the reference's test_extend_left_right (src/aligner.rs:603-639)
    const thm_mem hit{9, 6, 3};
    const auto lr = a.extend_left_right("AAAAAAACCTTGGGTTTTTTTT", hit, "GGGGCCTTGAGTAA", 1, 1, 4);
    std::printf("extend_left_right score=%d x=[%zu,%zu) y=[%zu,%zu) ops=%zu\n", lr.score, lr.xstart, lr.xend, lr.ystart, lr.yend,
                lr.operations.size());
    const std::string read = "ACGTACGTTTGACCA";
    const std::vector<thm_mem> mems = a.all_smems(read, 5);
    std::vector<std::uint32_t> bw(mems.size(), 5);
    std::vector<std::int32_t> xd(mems.size(), 5);
    std::vector<std::int32_t> status;
    const auto alns = a.align_seed_hits({read}, {mems}, bw, xd, 5, &status);
    std::printf("align_seed_hits: %zu hits\n", alns[0].size());
    return lr.score == 6 ? 0 : 1;
  } catch (const thermite::Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
