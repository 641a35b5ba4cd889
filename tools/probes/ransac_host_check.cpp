// Host check of the two-view RANSAC call's arithmetic (pislam_amd/csrc/pislam_geom_math.h, shared with the kernel), on
// the CPU only: reads pairs, runs pislam_two_view_ransac_batch's whole procedure serially (pgm::host_pair) and prints
// every output word.  tests/test_two_view.py compares the words with its numpy restatement of the header comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/ransac_host_check.cpp -o ransac_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   ransac_host_check cases.txt        (or the cases on standard input)
// One pair per line, whitespace separated decimal integers:
//   model hypotheses seed sigma_q8 b n  then per match: x1_q8 y1_q8 x2_q8 y2_q8
// (b is the pair's index in its batch, which the sampler hashes; n is what the call makes of counts[b] and stride:
// already clamped.)  One line of output per pair, floats as hexadecimal bit patterns:
//   best score ninliers inlier[n] as a string of 0 / 1 ("-" for n == 0) model_n[9] stats[8]
#include <vector>
#include "hex_words.h"
#include "pislam_geom_math.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int pairs = 0;
  for (;;) {
    int model, hypotheses;
    long long seed, sigma_q8, b, n;
    const int got = fscanf(f, "%d %d %lld %lld %lld %lld", &model, &hypotheses, &seed, &sigma_q8, &b, &n);
    if (got == EOF) break;
    if (got != 6 || (model != 0 && model != 1) || hypotheses < 1 || hypotheses > pgm::MAX_HYP || seed < 0 ||
        seed > 0xffffffffll || sigma_q8 < 1 || sigma_q8 > 4096 || b < 0 || b > 0x7fffffffll || n < 0 || n > pgm::MAX_STRIDE)
      return fprintf(stderr, "pair %d: bad header\n", pairs), 2;
    // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
    std::vector<int32_t> p1(2 * (size_t)n), p2(2 * (size_t)n);
    std::vector<uint8_t> inlier((size_t)n);
    for (long long i = 0; i < n; i++) {
      long long q[4];
      if (fscanf(f, "%lld %lld %lld %lld", &q[0], &q[1], &q[2], &q[3]) != 4) return fprintf(stderr, "pair %d: truncated\n", pairs), 2;
      p1[2 * (size_t)i] = (int32_t)q[0], p1[2 * (size_t)i + 1] = (int32_t)q[1];
      p2[2 * (size_t)i] = (int32_t)q[2], p2[2 * (size_t)i + 1] = (int32_t)q[3];
    }
    const pgm::PairIn I{p1.data(), p2.data(), (uint32_t)n, (uint32_t)b};
    pgm::PairOut O;
    if (model == 0)
      pgm::host_pair<0>(I, hypotheses, (uint32_t)seed, (int32_t)sigma_q8, &O, inlier.data());
    else
      pgm::host_pair<1>(I, hypotheses, (uint32_t)seed, (int32_t)sigma_q8, &O, inlier.data());
    printf("%" PRId32 " %" PRIu32 " %" PRIu32 " ", O.best, O.score, O.ninliers);
    if (n == 0) printf("-");
    for (long long i = 0; i < n; i++) putchar(inlier[(size_t)i] ? '1' : '0');
    for (int i = 0; i < 9; i++) pr_f32(O.model_n[i]);
    for (int i = 0; i < 8; i++) printf(" %lld", O.stats[i]);
    printf("\n");
    pairs++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
