// Sweep of the GEMM launch schedule (multimodal_llm_pretraining_amd/csrc/gemm_plan.h) on the
// host: for every legal problem of the grid below, under the default switches and each
// single-switch variant, the schedule mmpt_gemm_bf16 would execute must
//   - cover the M x N output exactly once with its launches' rectangles,
//   - split K in whole K-tiles: a split launch's kchunk is a multiple of 64 (an unsplit one's is K),
//     (splits - 1) * kchunk < K <= splits * kchunk, splits <= 16,
//   - use no more slab bytes than the workspace given (0, half, or all of the workspace query),
//   - touch / write no more C2 partial rows than the rows queries promise (for the problems the
//     queries describe: see `assumed` below),
//   - run gemm4p_kernel only where K % 64 == 0 and gemm4p_kt_kernel only for the K-tail forms,
//   - never walk K in reverse with the fused row sums,
//   - report tail_rows = the second launch's rows for the forward tail split, else 0.
// Exits non-zero with the offending problems printed.
//
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all
//       scripts/diag/gemm_plan_check.cpp -o gemm_plan_check; ./gemm_plan_check
#include <atomic>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>

#include "../../multimodal_llm_pretraining_amd/csrc/gemm_plan.h"

using namespace mmpt;

static std::atomic<long> fails{0}, checked{0};
static std::mutex print_mutex;

struct Variant {
  const char* name;
  GemmSwitches sw;
};

static void report(const char* what, const Variant& v, const GemmProblem& p) {
  if (fails.fetch_add(1) >= 20) return;
  std::lock_guard<std::mutex> lock(print_mutex);
  std::printf("FAIL %s [%s]: layouts %d/%d epilogue %d M %lld N %lld K %lld aligned %d workspace %lld\n",
              what, v.name, p.la, p.lb, p.epi, (long long)p.M, (long long)p.N, (long long)p.K,
              (int)p.aligned, (long long)p.ws_bytes);
}
#define CHECK(c) \
  do {           \
    if (!(c)) report(#c, v, p); \
  } while (0)

static void check_schedule(const Variant& v, const GemmProblem& p, int64_t ws_query,
                           int64_t cs_query, int64_t acs_query) {
  const GemmSchedule s = gemm_schedule(p, v.sw);
  CHECK(s.n == 1 || s.n == 2);
  CHECK(s.probe_after >= 0 && s.probe_after < s.n);
  int64_t area = 0;
  for (int i = 0; i < s.n; ++i) {
    const GemmLaunch& l = s.launch[i];
    CHECK(l.row0 >= 0 && l.col0 >= 0 && l.rows > 0 && l.cols > 0);
    CHECK(l.row0 + l.rows <= p.M && l.col0 + l.cols <= p.N);
    area += l.rows * l.cols;
    CHECK(l.splits >= 1 && l.splits <= 16);
    CHECK(l.splits > 1 ? l.kchunk % 64 == 0 : l.kchunk == p.K);
    CHECK((int64_t)(l.splits - 1) * l.kchunk < p.K && p.K <= (int64_t)l.splits * l.kchunk);
    CHECK((l.splits > 1) == (l.epi == EPI_SPLIT || l.epi == EPI_SPLIT_CS));
    CHECK(l.family != G4 || p.K % 64 == 0);
    CHECK(l.family != G4_KT || (p.K % 64 != 0 && kt_form(p.la, l.epi)));
    CHECK((l.tile == 256) == (l.family != G128));
    CHECK(l.tiles_m == (l.rows + l.tile - 1) / l.tile && l.tiles_n == (l.cols + l.tile - 1) / l.tile);
    CHECK(l.workgroups > 0 && l.group > 0);
    if (l.epi == MMPT_EPI_F32_ACC_COLSUM || l.epi == EPI_SPLIT_CS) CHECK(l.krev == 0);
  }
  CHECK(area == p.M * p.N);
  if (s.n == 2) {  // disjoint: stacked rows or side-by-side columns
    const GemmLaunch &a = s.launch[0], &b = s.launch[1];
    CHECK((a.col0 == b.col0 && a.cols == b.cols && a.row0 + a.rows == b.row0) ||
          (a.row0 == b.row0 && a.rows == b.rows && a.col0 + a.cols == b.col0));
  }
  CHECK((s.finish != FIN_NONE) == (s.launch[s.n - 1].splits > 1));
  CHECK(s.slab_bytes >= 0 && s.slab_bytes <= p.ws_bytes && p.ws_bytes <= ws_query);
  CHECK(s.tail_rows == (s.finish == FIN_TAIL_EPI ? s.launch[1].rows : 0));
  CHECK(s.finish != FIN_TAIL_EPI || (s.n == 2 && s.probe_after == 0));
  // The rows queries describe the assumed problem: 16-B aligned operands, K-contiguous for the
  // DGELU_COLSUM forms.  A DGELU_COLSUM call outside it may need more rows than the query
  // gives (gemm128's 128-row tiles where the query counted on gemm4p's); mmpt_gemm_bf16 refuses
  // such a call with an error, so those problems are not held to the bound here.
  const bool dgelu_cs = p.epi == MMPT_EPI_BF16_DGELU_COLSUM || p.epi == MMPT_EPI_BF16_DQGELU_COLSUM;
  const bool assumed = p.aligned && p.la == MMPT_ROWS_K && p.lb == MMPT_ROWS_K;
  if (dgelu_cs && assumed) CHECK(s.c2_rows_written <= cs_query && s.c2_rows <= cs_query);
  if (p.epi == MMPT_EPI_F32_ACC_COLSUM) CHECK(s.c2_rows_written <= acs_query && s.c2_rows <= acs_query);
  if (!dgelu_cs && p.epi != MMPT_EPI_F32_ACC_COLSUM) CHECK(s.c2_rows == 0 && s.c2_rows_written == 0);
}

static bool legal(int la, int lb, int epi, int64_t M, int64_t N, int64_t K) {
  if ((la == MMPT_K_ROWS ? M : K) % 8 != 0 || (lb == MMPT_K_ROWS ? N : K) % 8 != 0 || N % 4 != 0)
    return false;  // 16-byte DMA pieces: contiguous dims are multiples of 8
  if (epi == MMPT_EPI_BF16_SWIGLU && N % 256 != 0) return false;
  if (epi == MMPT_EPI_BF16_DSWIGLU && N % 128 != 0) return false;
  if (epi == MMPT_EPI_F32_ACC_COLSUM && !(la == MMPT_K_ROWS && lb == MMPT_K_ROWS)) return false;
  return true;
}

static void sweep_m(const std::vector<Variant>& variants, int64_t M) {
  const int64_t Ns[] = {256, 768, 2048, 3328, 6144, 8192, 50304};
  const int64_t Ks[] = {64, 1024, 2048, 8192, 8208, 22600, 69568, 180992};
  long n = 0;
  for (const Variant& v : variants)
    for (int64_t N : Ns)
      for (int64_t K : Ks) {
        const int64_t cs = gemm_colsum_rows(M, N, K, v.sw), acs = gemm_acc_colsum_rows(M, N, K, v.sw);
        for (int epi = 0; epi <= MMPT_EPI_F32_ACC_COLSUM; ++epi) {
          const int64_t wsq = gemm_workspace_bytes(M, N, K, epi, v.sw);
          for (int la = 0; la < 2; ++la)
            for (int lb = 0; lb < 2; ++lb) {
              if (!legal(la, lb, epi, M, N, K)) continue;
              for (int64_t ws : {(int64_t)0, wsq / 2, wsq})
                for (bool aligned : {true, false}) {
                  check_schedule(v, GemmProblem{la, lb, epi, M, N, K, aligned, ws, aligned}, wsq, cs, acs);
                  ++n;
                }
            }
        }
      }
  checked += n;
}

int main() {
  std::vector<Variant> variants;
  auto add = [&](const char* name, void (*set)(GemmSwitches&)) {
    Variant v{name, GemmSwitches{}};
    set(v.sw);
    variants.push_back(v);
  };
  add("default", [](GemmSwitches&) {});
  add("TAIL=0", [](GemmSwitches& s) { s.tail = 0; });
  add("TAIL128=0", [](GemmSwitches& s) { s.tail128 = 0; });
  add("WTAIL=0", [](GemmSwitches& s) { s.wtail = 0; });
  add("WTAIL=2", [](GemmSwitches& s) { s.wtail = 2; });
  add("PERSIST=0", [](GemmSwitches& s) { s.persist = 0; });
  add("4P=0", [](GemmSwitches& s) { s.g4 = 0; });
  add("cus=304", [](GemmSwitches& s) { s.cus = 304; });
  add("cus=64", [](GemmSwitches& s) { s.cus = 64; });
  add("KREV=1", [](GemmSwitches& s) { s.krev = 1; });  // (so that the row-sum check can fail)

  // M: multiples of 8 up to 9,216 and the M values of tests/golden/gemm_plan_table.json
  std::vector<int64_t> Ms;
  for (int64_t m = 8; m <= 9216; m += 8) Ms.push_back(m);
  for (int64_t m : {180992, 180224, 130816, 69568, 50432, 50304, 32784, 32512, 22624, 10240, 8804,
                    8292, 6304})
    Ms.push_back(m);

  const unsigned nt = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  std::atomic<size_t> next{0};
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < nt; ++t)
    pool.emplace_back([&] {
      for (size_t i; (i = next.fetch_add(1)) < Ms.size();) sweep_m(variants, Ms[i]);
    });
  for (std::thread& t : pool) t.join();
  std::printf(fails ? "gemm schedule: %ld schedules, %ld FAILURES\n" : "gemm schedule: %ld schedules ok\n",
              checked.load(), fails.load());
  return fails ? 1 : 0;
}
