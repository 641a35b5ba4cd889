// Host check of the Sim(3) RANSAC call's arithmetic (pislam_amd/csrc/pislam_sim3_math.h, shared with the kernel), on
// the CPU only: reads pairs, runs pislam_sim3_ransac_batch's whole procedure serially (s3m::host_pair) and prints every
// output word.  tests/test_sim3_ransac.py compares the words with its numpy restatement of the header comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/sim3_host_check.cpp -o sim3_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   sim3_host_check cases.txt        (or the cases on standard input)
// One pair per line, whitespace separated; floats are hexadecimal bit patterns, the rest decimal integers:
//   hypotheses seed min_inliers fixed_scale b has_level nlevels n  cam1[5] cam2[5] inv_sigma2[nlevels]
//   then per match: X1[3] X2[3]  u1_q8 v1_q8 w1_q8  u2_q8 v2_q8 w2_q8  level1 level2
// (b is the pair's index in its batch, which the sampler hashes; n is what the call makes of counts[b] and stride:
// already clamped; w1_q8, w2_q8 are the ignored third words.)  One line of output per pair:
//   best score ninliers status sim_out[13] inlier[n] as a string of 0 / 1 ("-" for n == 0)
#include <vector>
#include "hex_words.h"
#include "pislam_sim3_math.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int pairs = 0;
  for (;;) {
    int hypotheses, min_inliers, fixed_scale, has_level, nlevels;
    long long seed, b, n;
    const int got = fscanf(f, "%d %lld %d %d %lld %d %d %lld", &hypotheses, &seed, &min_inliers, &fixed_scale, &b, &has_level,
                           &nlevels, &n);
    if (got == EOF) break;
    if (got != 8 || hypotheses < 1 || hypotheses > s3m::MAX_HYP || seed < 0 || seed > 0xffffffffll || min_inliers < 3 ||
        min_inliers > s3m::MAX_STRIDE || fixed_scale < 0 || fixed_scale > 1 || b < 0 || b > 0x7fffffffll || nlevels < 0 ||
        nlevels > s3m::MAX_LEVELS || n < 0 || n > s3m::MAX_STRIDE || (has_level && nlevels < 1))
      return fprintf(stderr, "pair %d: bad header\n", pairs), 2;
    // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
    std::vector<float> cam1(5), cam2(5), tab((size_t)nlevels), x1(3 * (size_t)n), x2(3 * (size_t)n);
    std::vector<int32_t> obs1(3 * (size_t)n), obs2(3 * (size_t)n);
    std::vector<uint8_t> level1((size_t)n), level2((size_t)n), inlier((size_t)n);
    bool ok = true;
    for (auto &v : cam1) ok = ok && rd_f32(f, &v);
    for (auto &v : cam2) ok = ok && rd_f32(f, &v);
    for (auto &v : tab) ok = ok && rd_f32(f, &v);
    for (long long i = 0; ok && i < n; i++) {
      for (int k = 0; k < 3; k++) ok = ok && rd_f32(f, &x1[3 * (size_t)i + k]);
      for (int k = 0; k < 3; k++) ok = ok && rd_f32(f, &x2[3 * (size_t)i + k]);
      long long q[8];
      ok = ok && fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], &q[6], &q[7]) == 8;
      if (!ok) break;
      for (int k = 0; k < 3; k++) obs1[3 * (size_t)i + k] = (int32_t)q[k], obs2[3 * (size_t)i + k] = (int32_t)q[3 + k];
      level1[(size_t)i] = (uint8_t)q[6], level2[(size_t)i] = (uint8_t)q[7];
    }
    if (!ok) return fprintf(stderr, "pair %d: truncated\n", pairs), 2;
    s3m::Pair F;
    F.cam1 = cam1.data(), F.cam2 = cam2.data(), F.x1 = x1.data(), F.x2 = x2.data();
    F.obs1 = obs1.data(), F.obs2 = obs2.data();
    F.level1 = has_level ? level1.data() : nullptr, F.level2 = has_level ? level2.data() : nullptr;
    F.inv_sigma2 = has_level ? tab.data() : nullptr;
    F.nlevels = has_level ? nlevels : 0, F.n = (uint32_t)n, F.b = (uint32_t)b;
    s3m::Result R;
    s3m::host_pair(F, hypotheses, (uint32_t)seed, min_inliers, fixed_scale != 0, &R, inlier.data());
    printf("%" PRId32 " %" PRIu32 " %" PRIu32 " %" PRIu32, R.best, R.score, R.ninliers, R.status);
    for (int i = 0; i < s3m::OUT_WORDS; i++) pr_f32(R.sim[i]);
    printf(" ");
    if (n == 0) printf("-");
    for (long long i = 0; i < n; i++) putchar(inlier[(size_t)i] ? '1' : '0');
    printf("\n");
    pairs++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
