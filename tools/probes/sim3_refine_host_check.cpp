// Host check of the Sim(3) refinement's arithmetic (pislam_amd/csrc/pislam_sim3_refine_math.h, shared with the kernel),
// on the CPU only: reads pairs, runs pislam_sim3_refine_batch's whole procedure serially with the contract's tree order
// (s3r::host_pair) and prints every output word.  tests/test_sim3_refine.py compares the words with its numpy
// restatement of the header comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/sim3_refine_host_check.cpp -o sim3_refine_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   sim3_refine_host_check cases.txt        (or the cases on standard input)
// One pair per line, whitespace separated; floats are hexadecimal bit patterns (eps: 16 digits), the rest decimal:
//   rounds iters huber_rounds min_obs th2 fixed_scale eps has_level nlevels has_mask n
//   sim_in[13] cam1[5] cam2[5] inv_sigma2[nlevels]
//   then per match: X1[3] X2[3]  u1_q8 v1_q8 w1_q8  u2_q8 v2_q8 w2_q8  level1 level2 mask
// (n is what the call makes of counts[b] and stride: already clamped; w1_q8, w2_q8 are the ignored third words.)  One
// line of output per pair:
//   status ninliers cost sim_out[13] inlier[n] as a string of 0 / 1 ("-" for n == 0)
#include <vector>
#include "hex_words.h"
#include "pislam_sim3_refine_math.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int pairs = 0;
  for (;;) {
    s3r::Params P;
    int has_level, nlevels, has_mask;
    long long n;
    if (fscanf(f, "%d", &P.rounds) == EOF) break;
    uint64_t eps_bits = 0;
    bool ok = fscanf(f, "%d %d %d", &P.iters, &P.huber_rounds, &P.min_obs) == 3 && rd_f32(f, &P.th2) &&
              fscanf(f, "%d %" SCNx64 " %d %d %d %lld", &P.fixed_scale, &eps_bits, &has_level, &nlevels, &has_mask, &n) == 6;
    memcpy(&P.eps, &eps_bits, 8);
    if (!ok || P.rounds < 1 || P.rounds > 8 || P.iters < 1 || P.iters > 32 || P.huber_rounds < 0 || P.huber_rounds > P.rounds ||
        P.min_obs < 3 || P.min_obs > s3r::MAX_STRIDE || !(P.th2 > 0.0f) || !psm::finite_f(P.th2) || P.fixed_scale < 0 ||
        P.fixed_scale > 1 || !(P.eps >= 0.0) || nlevels < 0 || nlevels > s3r::MAX_LEVELS || n < 0 || n > s3r::MAX_STRIDE ||
        (has_level && nlevels < 1))
      return fprintf(stderr, "pair %d: bad header\n", pairs), 2;
    // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
    std::vector<float> sim(s3r::STATE), cam1(5), cam2(5), tab((size_t)nlevels), x1(3 * (size_t)n), x2(3 * (size_t)n);
    std::vector<int32_t> obs1(3 * (size_t)n), obs2(3 * (size_t)n);
    std::vector<uint8_t> level1((size_t)n), level2((size_t)n), mask((size_t)n), inlier((size_t)n);
    for (auto &v : sim) ok = ok && rd_f32(f, &v);
    for (auto &v : cam1) ok = ok && rd_f32(f, &v);
    for (auto &v : cam2) ok = ok && rd_f32(f, &v);
    for (auto &v : tab) ok = ok && rd_f32(f, &v);
    for (long long i = 0; ok && i < n; i++) {
      for (int k = 0; k < 3; k++) ok = ok && rd_f32(f, &x1[3 * (size_t)i + k]);
      for (int k = 0; k < 3; k++) ok = ok && rd_f32(f, &x2[3 * (size_t)i + k]);
      long long q[9];
      ok = ok && fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld %lld", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], &q[6], &q[7],
                        &q[8]) == 9;
      if (!ok) break;
      for (int k = 0; k < 3; k++) obs1[3 * (size_t)i + k] = (int32_t)q[k], obs2[3 * (size_t)i + k] = (int32_t)q[3 + k];
      level1[(size_t)i] = (uint8_t)q[6], level2[(size_t)i] = (uint8_t)q[7], mask[(size_t)i] = (uint8_t)q[8];
    }
    if (!ok) return fprintf(stderr, "pair %d: truncated\n", pairs), 2;
    s3r::Pair F;
    F.sim_in = sim.data(), F.mask = has_mask ? mask.data() : nullptr;
    F.m.cam1 = cam1.data(), F.m.cam2 = cam2.data(), F.m.x1 = x1.data(), F.m.x2 = x2.data();
    F.m.obs1 = obs1.data(), F.m.obs2 = obs2.data();
    F.m.level1 = has_level ? level1.data() : nullptr, F.m.level2 = has_level ? level2.data() : nullptr;
    F.m.inv_sigma2 = has_level ? tab.data() : nullptr;
    F.m.nlevels = has_level ? nlevels : 0, F.m.n = (uint32_t)n, F.m.b = 0;
    s3r::Result R;
    s3r::host_pair(F, P, &R, inlier.data());
    uint64_t cost_bits;
    memcpy(&cost_bits, &R.cost, 8);
    printf("%" PRIu32 " %" PRIu32 " %016" PRIx64, R.status, R.ninliers, cost_bits);
    for (int i = 0; i < s3r::STATE; i++) pr_f32(R.state[i]);
    printf(" ");
    if (n == 0) printf("-");
    for (long long i = 0; i < n; i++) putchar(inlier[(size_t)i] ? '1' : '0');
    printf("\n");
    pairs++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
