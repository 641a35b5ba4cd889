// Host check of the global bundle adjustment's arithmetic (pislam_amd/csrc/pislam_gba_math.h, shared with the kernels), on
// the CPU only: reads maps, runs pislam_global_ba_batch's whole procedure serially, phase by phase in the order of the
// launches (gba::host_map), and prints every output word.  tests/test_global_ba.py compares the words with its numpy
// restatement of the header comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/gba_host_check.cpp -o gba_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   gba_host_check cases.txt        (or the cases on standard input)
// One map per line, whitespace separated; floats are hexadecimal bit patterns, the rest decimal integers:
//   rounds iters[4] huber_rounds min_obs eps(64 bit) cg_iters cg_tol(64 bit) has_level nlevels
//   count kf_count npt stride kf_stride
//   inv_sigma2[nlevels]  per key frame: pose[12] cam[5] fixed   kf_ptr[nk + 1]   per point: X Y Z
//   per observation: kf pt  u_q8 v_q8 ur_q8  level  kf_obs
// count and kf_count are the signed words as given; the arrays hold n and nk entries, which are the counts if both are
// in range (0 <= count <= stride, 0 <= kf_count <= kf_stride) and 0 otherwise; npt is already clamped.  One line of output
// per map:
//   status ninliers cost(64 bit) poses_out[nk][12] xw_out[npt][3] inlier[n] as a string of 0 / 1 ("-" for n == 0)
//   solves cg_total fails rejects held (solves begun, PCG iterations, solves or steps that failed, steps that did not lower
//   F, the most points held in a solve), then the PCG iterations of every solve begun, joined by commas ("-" for none)
#include <vector>
#include "hex_words.h"
#include "pislam_gba_math.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int maps = 0;
  for (;;) {
    gba::Params P;
    uint64_t eps_bits, tol_bits;
    int has_level, nlevels;
    long long count, kf_count, npt, stride, kf_stride;
    const int got = fscanf(f, "%d %d %d %d %d %d %d %" SCNx64 " %d %" SCNx64 " %d %d %lld %lld %lld %lld %lld", &P.ba.rounds,
                           &P.ba.iters[0], &P.ba.iters[1], &P.ba.iters[2], &P.ba.iters[3], &P.ba.huber_rounds, &P.ba.min_obs,
                           &eps_bits, &P.cg_iters, &tol_bits, &has_level, &nlevels, &count, &kf_count, &npt, &stride, &kf_stride);
    if (got == EOF) break;
    bool hdr = got == 17 && stride >= 1 && stride <= (long long)gba::MAX_STRIDE && kf_stride >= 1 && kf_stride <= gba::MAX_KF &&
               npt >= 0 && npt <= (long long)gba::MAX_PTS && nlevels >= 0 && nlevels <= pq::MAX_LEVELS && P.ba.rounds >= 1 &&
               P.ba.rounds <= gba::MAX_ROUNDS && P.ba.huber_rounds >= 0 && P.ba.huber_rounds <= P.ba.rounds &&
               P.ba.min_obs >= 1 && P.cg_iters >= 1 && P.cg_iters <= gba::MAX_CG && count >= INT32_MIN && count <= INT32_MAX &&
               kf_count >= INT32_MIN && kf_count <= INT32_MAX;
    for (int r = 0; hdr && r < P.ba.rounds; r++) hdr = P.ba.iters[r] >= 1 && P.ba.iters[r] <= gba::MAX_ITERS;
    if (!hdr) return fprintf(stderr, "map %d: bad header\n", maps), 2;
    memcpy(&P.ba.eps, &eps_bits, 8);
    memcpy(&P.cg_tol, &tol_bits, 8);
    gba::Map M;
    gba::map_counts(M, (int32_t)count, (int32_t)kf_count, (uint32_t)npt, (size_t)stride, (size_t)kf_stride, (size_t)npt);
    const size_t n = M.n, nk = M.nk;
    // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
    std::vector<float> tab((size_t)nlevels), poses(12 * nk), cams(5 * nk), xw(3 * (size_t)npt);
    std::vector<int32_t> obs(3 * n), pt(n);
    std::vector<uint16_t> kf(n);
    std::vector<uint8_t> level(n), inlier(n), fixed(nk);
    std::vector<uint32_t> kf_ptr(nk + 1), kf_obs(n);
    bool ok = true;
    for (auto &v : tab) ok = ok && rd_f32(f, &v);
    for (size_t k = 0; ok && k < nk; k++) {
      for (int j = 0; j < 12; j++) ok = ok && rd_f32(f, &poses[12 * k + j]);
      for (int j = 0; j < 5; j++) ok = ok && rd_f32(f, &cams[5 * k + j]);
      int fx;
      ok = ok && fscanf(f, "%d", &fx) == 1;
      fixed[k] = ok ? (uint8_t)fx : 0;
    }
    for (auto &v : kf_ptr) ok = ok && fscanf(f, "%" SCNu32, &v) == 1;
    for (auto &v : xw) ok = ok && rd_f32(f, &v);
    for (size_t i = 0; ok && i < n; i++) {
      long long q[7];
      ok = ok && fscanf(f, "%lld %lld %lld %lld %lld %lld %lld", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], &q[6]) == 7;
      if (!ok) break;
      kf[i] = (uint16_t)q[0], pt[i] = (int32_t)q[1], level[i] = (uint8_t)q[5], kf_obs[i] = (uint32_t)q[6];
      for (int k = 0; k < 3; k++) obs[3 * i + k] = (int32_t)q[2 + k];
    }
    if (!ok) return fprintf(stderr, "map %d: truncated\n", maps), 2;
    M.poses = poses.data(), M.cams = cams.data(), M.xw = xw.data(), M.obs = obs.data(), M.pt = pt.data(), M.kf = kf.data();
    M.level = has_level ? level.data() : nullptr, M.fixed = fixed.data(), M.kf_ptr = kf_ptr.data(), M.kf_obs = kf_obs.data();
    M.W = pba::Window{};
    M.W.obs = M.obs, M.W.level = M.level, M.W.inv_sigma2 = has_level ? tab.data() : nullptr, M.W.nlevels = has_level ? nlevels : 0;
    std::vector<char> ws(gba::ws_bytes(nk, (size_t)npt, n) + 16);
    gba::ws_carve((char *)(((uintptr_t)ws.data() + 15) & ~(uintptr_t)15), nk, (size_t)npt, n, &M.ws);
    gba::Ctl C;
    memset(&C, 0, sizeof C);
    M.ctl = &C;
    std::vector<float> poses_out(12 * nk), xw_out(3 * (size_t)npt);
    std::vector<uint32_t> cg_log;
    gba::Result R;
    gba::host_map(M, P, poses_out.data(), xw_out.data(), inlier.data(), &R, &cg_log);
    uint64_t cost_bits;
    memcpy(&cost_bits, &R.cost, 8);
    printf("%" PRIu32 " %" PRIu32 " %016" PRIx64, R.status, R.ninliers, cost_bits);
    for (float v : poses_out) pr_f32(v);
    for (float v : xw_out) pr_f32(v);
    printf(" ");
    if (n == 0) printf("-");
    for (size_t i = 0; i < n; i++) putchar(inlier[i] ? '1' : '0');
    printf(" %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " ", R.solves, R.cg_total, R.fails, R.rejects, R.held);
    if (cg_log.empty()) printf("-");
    for (size_t i = 0; i < cg_log.size(); i++) printf(i ? ",%" PRIu32 : "%" PRIu32, cg_log[i]);
    printf("\n");
    maps++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
