// Host check of pislam_pose_graph_wide_batch: graph_host_check.cpp's graph mode with that call's limits (65536
// vertices, 2^20 edges).  The arithmetic is pgr::host_graph of pislam_amd/csrc/pislam_graph_math.h, which has no size
// limit of its own and which both device forms must equal bit for bit: this file is a main, not new arithmetic.
// tests/test_pose_graph_wide.py compares its lines with graph_host_check's and the device's words with its lines.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/graph_wide_host_check.cpp -o graph_wide_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   graph_wide_host_check cases.txt | cases.bin        (or text cases on standard input)
// Text: graph_host_check.cpp's `G` lines, one case per line (floats as hexadecimal bit patterns):
//   G iters cg_iters cg_tol(64 bit) eps(64 bit) has_weight nv ne
//     per vertex: fixed sims[13]   per edge: i j meas[13] weight   inc_ptr[nv + 1]   inc[2 ne]
// Binary (a text line of 2^20 edges is some 200 MB): raw little-endian arrays as numpy's tofile writes them, no padding:
//   the 8 bytes "PGWCASE1", uint32 cases, then per case
//   int32 iters, int32 cg_iters, float64 cg_tol, float64 eps, uint32 has_weight, uint32 nv, uint32 ne,
//   uint8 fixed[nv], float32 sims[nv][13], uint32 edges[ne][2], float32 meas[ne][13], float32 weight[ne] (only if
//   has_weight), uint32 inc_ptr[nv + 1], uint32 inc[2 ne]
// One line of output per case, as graph_host_check prints it:
//   status cost(64 bit) cg_iterations solves sims_out[nv][13]
#include <vector>
#include "hex_words.h"
#include "pislam_graph_math.h"

static const long long WIDE_MAX_V = 65536, WIDE_MAX_E = 1 << 20;

struct Case {
  pgr::Params P;
  int has_weight;
  std::vector<float> sims, meas, weight;
  std::vector<uint8_t> fixed;
  std::vector<uint32_t> edges, inc_ptr, inc;
  // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
  void size(long long nv, long long ne) {
    sims.resize(13 * (size_t)nv), meas.resize(13 * (size_t)ne), weight.resize((size_t)ne), fixed.resize((size_t)nv);
    edges.resize(2 * (size_t)ne), inc_ptr.resize((size_t)nv + 1), inc.resize(2 * (size_t)ne);
  }
};

static bool header_ok(const pgr::Params &P, long long nv, long long ne) {
  return nv >= 0 && nv <= WIDE_MAX_V && ne >= 0 && ne <= WIDE_MAX_E && P.iters >= 1 && P.iters <= 64 && P.cg_iters >= 1 &&
         P.cg_iters <= 1024;
}

static void run_case(const Case &c) {
  const size_t nv = c.fixed.size(), ne = c.weight.size();
  std::vector<float> out(13 * nv);
  std::vector<char> slice(pgr::ws_bytes(nv, ne) + 16, (char)0xff);   // (NaNs: nothing may rely on zeros)
  pgr::Graph G;
  G.sims = c.sims.data(), G.meas = c.meas.data(), G.weight = c.has_weight ? c.weight.data() : nullptr;
  G.fixed = c.fixed.data(), G.edges = c.edges.data(), G.inc_ptr = c.inc_ptr.data(), G.inc = c.inc.data();
  G.nv = (uint32_t)nv, G.ne = (uint32_t)ne;
  pgr::ws_carve((char *)(((uintptr_t)slice.data() + 15) & ~(uintptr_t)15), nv, ne, &G.ws);
  pgr::Result R;
  pgr::host_graph(G, c.P, out.data(), &R);
  uint64_t cost_bits;
  memcpy(&cost_bits, &R.cost, 8);
  printf("%" PRIu32 " %016" PRIx64 " %" PRIu32 " %" PRIu32, R.status, cost_bits, R.cg_total, R.solves);
  for (float v : out) pr_f32(v);
  printf("\n");
}

static bool rd_u32(FILE *f, uint32_t *v) {
  long long q;
  if (fscanf(f, "%lld", &q) != 1 || q < 0 || q > 0xffffffffll) return false;
  *v = (uint32_t)q;
  return true;
}

static int text_case(FILE *f, int cases) {
  Case c;
  uint64_t tol_bits, eps_bits;
  long long nv, ne;
  if (fscanf(f, "%d %d %" SCNx64 " %" SCNx64 " %d %lld %lld", &c.P.iters, &c.P.cg_iters, &tol_bits, &eps_bits, &c.has_weight,
             &nv, &ne) != 7 || !header_ok(c.P, nv, ne))
    return fprintf(stderr, "case %d: bad header\n", cases), 2;
  memcpy(&c.P.cg_tol, &tol_bits, 8), memcpy(&c.P.eps, &eps_bits, 8);
  c.size(nv, ne);
  bool ok = true;
  for (long long k = 0; ok && k < nv; k++) {
    uint32_t fx;
    ok = rd_u32(f, &fx);
    c.fixed[(size_t)k] = (uint8_t)fx;
    for (int j = 0; j < 13; j++) ok = ok && rd_f32(f, &c.sims[13 * (size_t)k + j]);
  }
  for (long long e = 0; ok && e < ne; e++) {
    ok = rd_u32(f, &c.edges[2 * (size_t)e]) && rd_u32(f, &c.edges[2 * (size_t)e + 1]);
    for (int j = 0; j < 13; j++) ok = ok && rd_f32(f, &c.meas[13 * (size_t)e + j]);
    ok = ok && rd_f32(f, &c.weight[(size_t)e]);
  }
  for (auto &v : c.inc_ptr) ok = ok && rd_u32(f, &v);
  for (auto &v : c.inc) ok = ok && rd_u32(f, &v);
  if (!ok) return fprintf(stderr, "case %d: truncated\n", cases), 2;
  run_case(c);
  return 0;
}

template <class T>
static bool rd_raw(FILE *f, std::vector<T> &v) {
  return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

static int binary_case(FILE *f, int cases) {
  Case c;
  int32_t it[2];
  double tol[2];
  uint32_t n[3];
  if (fread(it, 4, 2, f) != 2 || fread(tol, 8, 2, f) != 2 || fread(n, 4, 3, f) != 3)
    return fprintf(stderr, "case %d: truncated\n", cases), 2;
  c.P = pgr::Params{it[0], it[1], tol[0], tol[1]}, c.has_weight = n[0] != 0;
  if (!header_ok(c.P, n[1], n[2])) return fprintf(stderr, "case %d: bad header\n", cases), 2;
  c.size(n[1], n[2]);
  bool ok = rd_raw(f, c.fixed) && rd_raw(f, c.sims) && rd_raw(f, c.edges) && rd_raw(f, c.meas);
  if (c.has_weight) ok = ok && rd_raw(f, c.weight);
  ok = ok && rd_raw(f, c.inc_ptr) && rd_raw(f, c.inc);
  if (!ok) return fprintf(stderr, "case %d: truncated\n", cases), 2;
  run_case(c);
  return 0;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  static const char MAGIC[] = "PGWCASE1";
  const int first = fgetc(f);
  if (first == MAGIC[0]) {
    char rest[7];
    uint32_t cases;
    if (fread(rest, 1, 7, f) != 7 || memcmp(rest, MAGIC + 1, 7) != 0 || fread(&cases, 4, 1, f) != 1)
      return fprintf(stderr, "bad binary header\n"), 2;
    for (uint32_t i = 0; i < cases; i++)
      if (const int rc = binary_case(f, (int)i)) return rc;
    return 0;
  }
  if (first != EOF) ungetc(first, f);
  int cases = 0;
  for (;;) {
    char mode[2];
    const int got = fscanf(f, "%1s", mode);
    if (got == EOF) break;
    if (mode[0] != 'G') return fprintf(stderr, "case %d: unknown mode (this probe takes graphs only)\n", cases), 2;
    if (const int rc = text_case(f, cases)) return rc;
    cases++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
