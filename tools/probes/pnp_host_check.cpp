// Host check of the absolute-pose RANSAC call's arithmetic (pislam_amd/csrc/pislam_pnp_math.h, shared with the
// kernel), on the CPU only: reads frames, runs pislam_pnp_ransac_batch's whole procedure serially (pnm::host_frame) and
// prints every output word.  tests/test_pnp_ransac.py compares the words with its numpy restatement of the header
// comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/pnp_host_check.cpp -o pnp_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   pnp_host_check cases.txt        (or the cases on standard input)
// One frame per line, whitespace separated; floats are hexadecimal bit patterns, the rest decimal integers:
//   hypotheses seed min_inliers b has_level nlevels n  cam[5] inv_sigma2[nlevels]
//   then per observation: X Y Z  u_q8 v_q8 ur_q8  level
// (b is the frame's index in its batch, which the sampler hashes; n is what the call makes of counts[b] and stride:
// already clamped.)  One line of output per frame:
//   best score ninliers status pose_out[12] inlier[n] as a string of 0 / 1 ("-" for n == 0)
#include <vector>
#include "hex_words.h"
#include "pislam_pnp_math.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int frames = 0;
  for (;;) {
    int hypotheses, min_inliers, has_level, nlevels;
    long long seed, b, n;
    const int got = fscanf(f, "%d %lld %d %lld %d %d %lld", &hypotheses, &seed, &min_inliers, &b, &has_level, &nlevels, &n);
    if (got == EOF) break;
    if (got != 7 || hypotheses < 1 || hypotheses > pnm::MAX_HYP || seed < 0 || seed > 0xffffffffll || min_inliers < 4 ||
        min_inliers > pnm::MAX_STRIDE || b < 0 || b > 0x7fffffffll || nlevels < 0 || nlevels > pnm::MAX_LEVELS || n < 0 ||
        n > pnm::MAX_STRIDE || (has_level && nlevels < 1))
      return fprintf(stderr, "frame %d: bad header\n", frames), 2;
    // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
    std::vector<float> cam(5), tab((size_t)nlevels), xw(3 * (size_t)n);
    std::vector<int32_t> obs(3 * (size_t)n);
    std::vector<uint8_t> level((size_t)n), inlier((size_t)n);
    bool ok = true;
    for (auto &v : cam) ok = ok && rd_f32(f, &v);
    for (auto &v : tab) ok = ok && rd_f32(f, &v);
    for (long long i = 0; ok && i < n; i++) {
      for (int k = 0; k < 3; k++) ok = ok && rd_f32(f, &xw[3 * (size_t)i + k]);
      long long q[4];
      ok = ok && fscanf(f, "%lld %lld %lld %lld", &q[0], &q[1], &q[2], &q[3]) == 4;
      if (!ok) break;
      for (int k = 0; k < 3; k++) obs[3 * (size_t)i + k] = (int32_t)q[k];
      level[(size_t)i] = (uint8_t)q[3];
    }
    if (!ok) return fprintf(stderr, "frame %d: truncated\n", frames), 2;
    pnm::Frame F;
    F.cam = cam.data(), F.xw = xw.data(), F.obs = obs.data();
    F.level = has_level ? level.data() : nullptr, F.inv_sigma2 = has_level ? tab.data() : nullptr;
    F.nlevels = has_level ? nlevels : 0, F.n = (uint32_t)n, F.b = (uint32_t)b;
    pnm::Result R;
    pnm::host_frame(F, hypotheses, (uint32_t)seed, min_inliers, &R, inlier.data());
    printf("%" PRId32 " %" PRIu32 " %" PRIu32 " %" PRIu32, R.best, R.score, R.ninliers, R.status);
    for (int i = 0; i < 12; i++) pr_f32(R.pose[i]);
    printf(" ");
    if (n == 0) printf("-");
    for (long long i = 0; i < n; i++) putchar(inlier[(size_t)i] ? '1' : '0');
    printf("\n");
    frames++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
