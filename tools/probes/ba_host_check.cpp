// Host check of the local bundle adjustment's arithmetic (pislam_amd/csrc/pislam_ba_math.h, shared with the kernel), on
// the CPU only: reads windows, runs pislam_local_ba_batch's whole procedure serially in the contract's orders
// (pba::host_window) and prints every output word.  tests/test_local_ba.py compares the words with its numpy
// restatement of the header comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/ba_host_check.cpp -o ba_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   ba_host_check cases.txt        (or the cases on standard input)
// One window per line, whitespace separated; floats are hexadecimal bit patterns, the rest decimal integers:
//   rounds iters[4] huber_rounds min_obs eps(64 bit) has_level nlevels nkf nfree npt n
//   inv_sigma2[nlevels]  per key frame: pose[12] cam[5]  per point: X Y Z
//   per observation: kf pt  u_q8 v_q8 ur_q8  level
// (nkf, npt and n are what the call makes of the counts and strides: already clamped; nfree is kf_free as given.)  One
// line of output per window:
//   status ninliers cost(64 bit) poses_out[nkf][12] xw_out[npt][3] inlier[n] as a string of 0 / 1 ("-" for n == 0)
#include <vector>
#include "hex_words.h"
#include "pislam_ba_math.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int windows = 0;
  for (;;) {
    pba::Params P;
    uint64_t eps_bits;
    int has_level, nlevels;
    long long nkf, nfree, npt, n;
    const int got = fscanf(f, "%d %d %d %d %d %d %d %" SCNx64 " %d %d %lld %lld %lld %lld", &P.rounds, &P.iters[0], &P.iters[1],
                           &P.iters[2], &P.iters[3], &P.huber_rounds, &P.min_obs, &eps_bits, &has_level, &nlevels, &nkf,
                           &nfree, &npt, &n);
    if (got == EOF) break;
    bool hdr = got == 14 && n >= 0 && n <= pba::MAX_STRIDE && nkf >= 0 && nkf <= pba::MAX_KF && npt >= 0 &&
               npt <= pba::MAX_PTS && nfree >= 0 && nlevels >= 0 && nlevels <= pq::MAX_LEVELS && P.rounds >= 1 &&
               P.rounds <= pba::MAX_ROUNDS && P.huber_rounds >= 0 && P.huber_rounds <= P.rounds && P.min_obs >= 1;
    for (int r = 0; hdr && r < P.rounds; r++) hdr = P.iters[r] >= 1 && P.iters[r] <= 32;
    if (!hdr) return fprintf(stderr, "window %d: bad header\n", windows), 2;
    memcpy(&P.eps, &eps_bits, 8);
    // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
    std::vector<float> tab((size_t)nlevels), poses(12 * (size_t)nkf), cams(5 * (size_t)nkf), xw(3 * (size_t)npt);
    std::vector<int32_t> obs(3 * (size_t)n);
    std::vector<uint8_t> kf((size_t)n), level((size_t)n), inlier((size_t)n);
    std::vector<uint16_t> pt((size_t)n);
    bool ok = true;
    for (auto &v : tab) ok = ok && rd_f32(f, &v);
    for (long long k = 0; ok && k < nkf; k++) {
      for (int j = 0; j < 12; j++) ok = ok && rd_f32(f, &poses[12 * (size_t)k + j]);
      for (int j = 0; j < 5; j++) ok = ok && rd_f32(f, &cams[5 * (size_t)k + j]);
    }
    for (auto &v : xw) ok = ok && rd_f32(f, &v);
    for (long long i = 0; ok && i < n; i++) {
      long long q[6];
      ok = ok && fscanf(f, "%lld %lld %lld %lld %lld %lld", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5]) == 6;
      if (!ok) break;
      kf[(size_t)i] = (uint8_t)q[0], pt[(size_t)i] = (uint16_t)q[1], level[(size_t)i] = (uint8_t)q[5];
      for (int k = 0; k < 3; k++) obs[3 * (size_t)i + k] = (int32_t)q[2 + k];
    }
    if (!ok) return fprintf(stderr, "window %d: truncated\n", windows), 2;
    pba::Window W;
    W.poses = poses.data(), W.cams = cams.data(), W.xw = xw.data(), W.obs = obs.data(), W.kf = kf.data(), W.pt = pt.data();
    W.level = has_level ? level.data() : nullptr, W.inv_sigma2 = has_level ? tab.data() : nullptr;
    W.nlevels = has_level ? nlevels : 0;
    W.nkf = (uint32_t)nkf, W.nfree = (uint32_t)nfree, W.npt = (uint32_t)npt, W.n = (uint32_t)n;
    std::vector<float> poses_out(12 * (size_t)nkf), xw_out(3 * (size_t)npt);
    pba::Result R;
    pba::host_window(W, P, poses_out.data(), xw_out.data(), inlier.data(), &R);
    uint64_t cost_bits;
    memcpy(&cost_bits, &R.cost, 8);
    printf("%" PRIu32 " %" PRIu32 " %016" PRIx64, R.status, R.ninliers, cost_bits);
    for (float v : poses_out) pr_f32(v);
    for (float v : xw_out) pr_f32(v);
    printf(" ");
    if (n == 0) printf("-");
    for (long long i = 0; i < n; i++) putchar(inlier[(size_t)i] ? '1' : '0');
    printf("\n");
    windows++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
