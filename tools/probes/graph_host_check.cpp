// Host check of the essential-graph optimisation's arithmetic (pislam_amd/csrc/pislam_graph_math.h, shared with the
// kernels), on the CPU only: reads graphs, runs pislam_pose_graph_batch's whole procedure serially in the contract's
// orders (pgr::host_graph) and prints every output word; a second mode does the same for
// pislam_map_points_correct_batch.  tests/test_pose_graph.py compares the words with its numpy restatement of the header
// comments.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/graph_host_check.cpp -o graph_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   graph_host_check cases.txt        (or the cases on standard input)
// One case per line, whitespace separated; floats are hexadecimal bit patterns, the rest decimal integers.
//   G iters cg_iters cg_tol(64 bit) eps(64 bit) has_weight nv ne
//     per vertex: fixed sims[13]   per edge: i j meas[13] weight   inc_ptr[nv + 1]   inc[2 ne]
//   P nv npt   sims_old[nv][13]   sims_new[nv][13]   per point: ref X Y Z
// (nv, ne and npt are what the call makes of the counts and strides: already clamped.)  One line of output per case:
//   G: status cost(64 bit) cg_iterations solves sims_out[nv][13]      P: per point status X' Y' Z'
#include <vector>
#include "hex_words.h"
#include "pislam_graph_math.h"

static bool rd_u32(FILE *f, uint32_t *v) {
  long long q;
  if (fscanf(f, "%lld", &q) != 1 || q < 0 || q > 0xffffffffll) return false;
  *v = (uint32_t)q;
  return true;
}

static int graph_case(FILE *f, int cases) {
  pgr::Params P;
  uint64_t tol_bits, eps_bits;
  int has_weight;
  long long nv, ne;
  if (fscanf(f, "%d %d %" SCNx64 " %" SCNx64 " %d %lld %lld", &P.iters, &P.cg_iters, &tol_bits, &eps_bits, &has_weight,
             &nv, &ne) != 7 ||
      nv < 0 || nv > pgr::MAX_V || ne < 0 || ne > pgr::MAX_E || P.iters < 1 || P.iters > 64 || P.cg_iters < 1 ||
      P.cg_iters > 1024)
    return fprintf(stderr, "case %d: bad header\n", cases), 2;
  memcpy(&P.cg_tol, &tol_bits, 8), memcpy(&P.eps, &eps_bits, 8);
  // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
  std::vector<float> sims(13 * (size_t)nv), meas(13 * (size_t)ne), weight((size_t)ne), out(13 * (size_t)nv);
  std::vector<uint8_t> fixed((size_t)nv);
  std::vector<uint32_t> edges(2 * (size_t)ne), inc_ptr((size_t)nv + 1), inc(2 * (size_t)ne);
  bool ok = true;
  for (long long k = 0; ok && k < nv; k++) {
    uint32_t fx;
    ok = rd_u32(f, &fx);
    fixed[(size_t)k] = (uint8_t)fx;
    for (int j = 0; j < 13; j++) ok = ok && rd_f32(f, &sims[13 * (size_t)k + j]);
  }
  for (long long e = 0; ok && e < ne; e++) {
    ok = rd_u32(f, &edges[2 * (size_t)e]) && rd_u32(f, &edges[2 * (size_t)e + 1]);
    for (int j = 0; j < 13; j++) ok = ok && rd_f32(f, &meas[13 * (size_t)e + j]);
    ok = ok && rd_f32(f, &weight[(size_t)e]);
  }
  for (auto &v : inc_ptr) ok = ok && rd_u32(f, &v);
  for (auto &v : inc) ok = ok && rd_u32(f, &v);
  if (!ok) return fprintf(stderr, "case %d: truncated\n", cases), 2;
  std::vector<char> slice(pgr::ws_bytes((size_t)nv, (size_t)ne) + 16, (char)0xff);   // (NaNs: nothing may rely on zeros)
  pgr::Graph G;
  G.sims = sims.data(), G.meas = meas.data(), G.weight = has_weight ? weight.data() : nullptr, G.fixed = fixed.data();
  G.edges = edges.data(), G.inc_ptr = inc_ptr.data(), G.inc = inc.data(), G.nv = (uint32_t)nv, G.ne = (uint32_t)ne;
  pgr::ws_carve((char *)(((uintptr_t)slice.data() + 15) & ~(uintptr_t)15), (size_t)nv, (size_t)ne, &G.ws);
  pgr::Result R;
  pgr::host_graph(G, P, out.data(), &R);
  uint64_t cost_bits;
  memcpy(&cost_bits, &R.cost, 8);
  printf("%" PRIu32 " %016" PRIx64 " %" PRIu32 " %" PRIu32, R.status, cost_bits, R.cg_total, R.solves);
  for (float v : out) pr_f32(v);
  printf("\n");
  return 0;
}

static int points_case(FILE *f, int cases) {
  long long nv, npt;
  if (fscanf(f, "%lld %lld", &nv, &npt) != 2 || nv < 0 || nv > 65536 || npt < 0)
    return fprintf(stderr, "case %d: bad header\n", cases), 2;
  std::vector<float> so(13 * (size_t)nv), sn(13 * (size_t)nv);
  bool ok = true;
  for (auto &v : so) ok = ok && rd_f32(f, &v);
  for (auto &v : sn) ok = ok && rd_f32(f, &v);
  for (long long p = 0; ok && p < npt; p++) {
    uint32_t ref;
    float X[3], Y[3];
    ok = rd_u32(f, &ref) && rd_f32(f, &X[0]) && rd_f32(f, &X[1]) && rd_f32(f, &X[2]);
    if (!ok) break;
    Y[0] = X[0], Y[1] = X[1], Y[2] = X[2];
    const bool moved = ref < (uint32_t)nv && pgr::correct_point(&so[13 * (size_t)ref], &sn[13 * (size_t)ref], X, Y);
    printf("%s%d", p ? " " : "", moved ? 0 : 1);
    for (float v : Y) pr_f32(v);
  }
  if (!ok) return fprintf(stderr, "case %d: truncated\n", cases), 2;
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int cases = 0;
  for (;;) {
    char mode[2];
    const int got = fscanf(f, "%1s", mode);
    if (got == EOF) break;
    int rc = 2;
    if (mode[0] == 'G') rc = graph_case(f, cases);
    else if (mode[0] == 'P') rc = points_case(f, cases);
    else fprintf(stderr, "case %d: unknown mode\n", cases);
    if (rc) return rc;
    cases++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
