// Host restatement of the work-item enumeration of the varlen attention kernels
// (csrc/attention.hip: attn_item + item_at of the persistent forward / dQ kernels, the
// (key block, batch·kv head) grid of the ring dK/dV kernel, the (b, q, h) rows of the δ
// kernel) for ragged length lists.  Checks that every (sequence, head, block) with rows is
// visited exactly once, that an empty item is never decoded into loads (the next-item K/V
// prefetch included), and that every token row a visited item loads or stores lies inside its
// own sequence [cu[b], cu[b+1]).
//
//   g++ -O1 -g -fsanitize=address,undefined scripts/diag/varlen_items_check.cpp -o varlen_items_check
//   ./varlen_items_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <vector>

static int fails = 0;
#define CHECK(c, ...)                       \
  do {                                      \
    if (!(c)) {                             \
      if (++fails < 20) {                   \
        std::printf("FAIL %s: ", #c);       \
        std::printf(__VA_ARGS__);           \
        std::printf("\n");                  \
      }                                     \
    }                                       \
  } while (0)

// attn_item with gridDim.x = G, blockIdx.x = bid
static int attn_item(int G, int bid, int n, int k) {
  const int q8 = n >> 3, r8 = n & 7;
  auto start = [&](int x) { return x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8; };
  if (G >= n) return k == 0 && bid < n ? start(bid & 7) + (bid >> 3) : -1;
  const int x = bid & 7, j = bid >> 3, W = G >> 3;
  const int local = k * W + ((k & 1) ? W - 1 - j : j);
  return local < q8 + (x < r8 ? 1 : 0) ? start(x) + local : -1;
}

struct Geo {
  std::vector<int> cu;
  int B, H, S;  // S = max_seq
  int len(int b) const { return cu[b + 1] - cu[b]; }
};

static void row_ok(const Geo& g, int b, long row, const char* what) {
  CHECK(row >= g.cu[b] && row < g.cu[b + 1], "%s row %ld outside [%d, %d) of sequence %d", what, row,
        g.cu[b], g.cu[b + 1], b);
}

// persistent forward / dQ: BQ query rows per item, 64-key blocks
static void check_persistent(const Geo& g, int BQ, bool causal, int G) {
  const int nx = (g.S + BQ - 1) / BQ, n = nx * g.B * g.H;
  const int grid = G > 0 && n > G ? G : n;
  std::map<std::tuple<int, int, int>, int> seen;
  for (int bid = 0; bid < grid; ++bid) {
    auto item_at = [&](int& k) {
      for (;; ++k) {
        const int w = attn_item(grid, bid, n, k);
        if (w < 0) return w;
        if ((nx - 1 - w % nx) * BQ < g.len(w / nx / g.H)) return w;
      }
    };
    auto stage = [&](int b, int kb) {  // the rows a K/V block DMA touches
      CHECK(kb * 64 < g.len(b), "staged key block %d of sequence %d (len %d) is empty", kb, b, g.len(b));
      for (int r = 0; r < 64; ++r)
        row_ok(g, b, (long)g.cu[b] + std::min(kb * 64 + r, g.len(b) - 1), "kv");
    };
    int it = 0;
    int wid = item_at(it);
    bool first = true;
    while (wid >= 0) {
      const int bx = nx - 1 - wid % nx, bh = wid / nx, b = bh / g.H, h = bh % g.H, q0 = bx * BQ;
      const int S = g.len(b);
      CHECK(q0 < S, "empty item visited: b %d q0 %d len %d", b, q0, S);
      ++seen[{b, h, bx}];
      const int nkb_s = (S + 63) / 64;
      const int nkb = causal ? std::min(nkb_s, (q0 + BQ - 1) / 64 + 1) : nkb_s;
      CHECK(nkb >= 1, "item without key blocks");
      for (int r = 0; r < BQ; ++r) {
        row_ok(g, b, (long)g.cu[b] + std::min(q0 + r, S - 1), "q");
        if (q0 + r < S) row_ok(g, b, (long)g.cu[b] + q0 + r, "store");
      }
      if (first) stage(b, 0);
      first = false;
      int itn = it + 1;
      const int wid_n = item_at(itn);
      for (int kb = 0; kb < nkb; ++kb) {
        if (kb + 1 < nkb) stage(b, kb + 1);
        else if (wid_n >= 0) stage(wid_n / nx / g.H, 0);
      }
      wid = wid_n;
      it = itn;
    }
  }
  for (int b = 0; b < g.B; ++b)
    for (int h = 0; h < g.H; ++h)
      for (int bx = 0; bx < nx; ++bx) {
        const int want = bx * BQ < g.len(b) ? 1 : 0;
        const auto f = seen.find({b, h, bx});
        const int got = f == seen.end() ? 0 : f->second;
        CHECK(got == want, "item (b %d, h %d, bx %d) visited %d times, want %d (BQ %d grid %d)", b, h, bx,
              got, want, BQ, grid);
      }
}

// ring dK/dV: KB keys per workgroup, 32-query blocks; grid (ceil(S/KB), B * Hkv)
static void check_ring(const Geo& g, int KB, bool causal) {
  const int nxb = (g.S + KB - 1) / KB;
  for (int b = 0; b < g.B; ++b) {
    const int S = g.len(b);
    std::vector<int> cover(S, 0);
    for (int bx = 0; bx < nxb; ++bx) {
      const int k0 = bx * KB;
      if (k0 >= S) continue;  // the kernel's uniform early exit
      const int nqb = (S + 31) / 32, qb0 = causal ? k0 / 32 : 0, cnt = nqb - qb0;
      CHECK(cnt >= 1, "key block %d of sequence %d sweeps no query block", bx, b);
      for (int r = 0; r < KB; ++r) {
        row_ok(g, b, (long)g.cu[b] + std::min(k0 + r, S - 1), "k");
        if (k0 + r < S) ++cover[k0 + r];
      }
      for (int qb = qb0; qb < nqb; ++qb)
        for (int r = 0; r < 32; ++r) {
          row_ok(g, b, (long)g.cu[b] + std::min(qb * 32 + r, S - 1), "q/dO");
          const int q = std::min(qb * 32 + r, S - 1);
          CHECK(q >= 0 && q < g.S, "lse / delta index %d outside [0, %d)", q, g.S);
        }
    }
    for (int k = 0; k < S; ++k) CHECK(cover[k] == 1, "key %d of sequence %d written %d times", k, b, cover[k]);
  }
}

// δ: rows over (b, q < max_seq, h)
static void check_delta(const Geo& g) {
  std::vector<int> cover(g.cu[g.B], 0);
  for (long row = 0; row < (long)g.B * g.S * g.H; ++row) {
    const long t = row / g.H;
    const int b = (int)(t / g.S), q = (int)(t % g.S);
    if (q >= g.len(b)) continue;
    row_ok(g, b, (long)g.cu[b] + q, "delta");
    if (row % g.H == 0) ++cover[g.cu[b] + q];
  }
  for (int t = 0; t < g.cu[g.B]; ++t) CHECK(cover[t] == 1, "token %d covered %d times by delta", t, cover[t]);
}

int main() {
  const std::vector<std::vector<int>> lists = {
      {1, 64, 65, 200}, {1, 70, 128, 129, 257}, {200, 1, 1, 1}, {1}, {257}, {64, 64, 64},
      {1, 1, 1, 1, 1, 1, 1, 1, 1, 300}, {33, 2, 511, 512, 513, 17}};
  std::srand(7);
  std::vector<std::vector<int>> all = lists;
  for (int i = 0; i < 40; ++i) {
    std::vector<int> l(1 + std::rand() % 9);
    for (int& x : l) x = 1 + std::rand() % 700;
    all.push_back(l);
  }
  for (const auto& l : all) {
    for (int H : {1, 3, 4}) {
      Geo g;
      g.B = (int)l.size();
      g.H = H;
      g.cu.assign(1, 0);
      for (int x : l) g.cu.push_back(g.cu.back() + x);
      const int mx = *std::max_element(l.begin(), l.end());
      for (int S : {mx, mx + 37}) {
        g.S = S;
        for (bool causal : {false, true}) {
          for (int BQ : {64, 128})
            for (int G : {0, 8, 16, 256}) check_persistent(g, BQ, causal, G);
          for (int KB : {64, 128}) check_ring(g, KB, causal);
        }
        check_delta(g);
      }
    }
  }
  std::printf(fails ? "varlen item enumeration: %d FAILURES\n" : "varlen item enumeration: ok\n", fails);
  return fails ? 1 : 0;
}
