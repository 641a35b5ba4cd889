// Host check of the pose call's arithmetic (pislam_amd/csrc/pislam_pose_math.h, shared with the kernel), on the CPU
// only: reads frames, runs pislam_pose_refine_batch's whole procedure serially with the contract's tree order
// (pq::host_frame) and prints every output word.  tests/test_pose_refine.py compares the words with its numpy
// restatement of the header comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/pose_host_check.cpp -o pose_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   pose_host_check cases.txt        (or the cases on standard input)
// One frame per line, whitespace separated; floats are hexadecimal bit patterns, the rest decimal integers:
//   rounds iters huber_rounds min_obs eps(64 bit) has_level nlevels n  pose[12] cam[5] inv_sigma2[nlevels]
//   then per observation: X Y Z  u_q8 v_q8 ur_q8  level
// (n is what the call makes of counts[b] and stride: already clamped.)  One line of output per frame:
//   status ninliers cost(64 bit) pose_out[12] inlier[n] as a string of 0 / 1 ("-" for n == 0)
#include <vector>
#include "hex_words.h"
#include "pislam_pose_math.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int frames = 0;
  for (;;) {
    pq::Params P;
    uint64_t eps_bits;
    int has_level, nlevels;
    long long n;
    const int got = fscanf(f, "%d %d %d %d %" SCNx64 " %d %d %lld", &P.rounds, &P.iters, &P.huber_rounds, &P.min_obs,
                           &eps_bits, &has_level, &nlevels, &n);
    if (got == EOF) break;
    if (got != 8 || n < 0 || n > pq::MAX_STRIDE || nlevels < 0 || nlevels > pq::MAX_LEVELS || P.rounds < 1 ||
        P.rounds > 8 || P.iters < 1 || P.iters > 32 || P.huber_rounds < 0 || P.huber_rounds > P.rounds || P.min_obs < 3)
      return fprintf(stderr, "frame %d: bad header\n", frames), 2;
    memcpy(&P.eps, &eps_bits, 8);
    // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
    std::vector<float> pose(12), cam(5), tab((size_t)nlevels), xw(3 * (size_t)n);
    std::vector<int32_t> obs(3 * (size_t)n);
    std::vector<uint8_t> level((size_t)n), inlier((size_t)n);
    bool ok = true;
    for (auto &v : pose) ok = ok && rd_f32(f, &v);
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
    pq::Frame F;
    F.pose_in = pose.data(), F.cam = cam.data(), F.xw = xw.data(), F.obs = obs.data();
    F.level = has_level ? level.data() : nullptr, F.inv_sigma2 = has_level ? tab.data() : nullptr;
    F.nlevels = has_level ? nlevels : 0, F.n = (uint32_t)n;
    pq::Result R;
    pq::host_frame(F, P, &R, inlier.data());
    uint64_t cost_bits;
    memcpy(&cost_bits, &R.cost, 8);
    printf("%" PRIu32 " %" PRIu32 " %016" PRIx64, R.status, R.ninliers, cost_bits);
    for (int i = 0; i < 12; i++) pr_f32(R.state[i]);
    printf(" ");
    if (n == 0) printf("-");
    for (long long i = 0; i < n; i++) putchar(inlier[(size_t)i] ? '1' : '0');
    printf("\n");
    frames++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
