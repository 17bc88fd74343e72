// Runs the replay form of the SemiLG state kernels - magat_sim_replayed_states (csrc/sim_guidance.hip) and
// magat_sim_replayed_states_wide (csrc/sim_guidance_wide.hip) - on the host, one thread per lane of their one-wave workgroups
// (hip/hip_runtime.h next to this file), without a GPU:
//   c++ -std=c++17 -O1 -g -pthread -I tools/host_wave -x c++ tools/host_wave/semi_replay_check.cpp -o semi_replay_check
//   semi_replay_check case.txt > result.txt
// (add -fsanitize=address,undefined to have every access of the kernel checked: every buffer here has exactly its documented
// size, the wide form's workspace included.)  case.txt: whitespace-separated integers B N H W FOV wide has_table cases T Lcap,
// then the maps (B H W), pos (B N 2), goal (B N 2), row_case (B), row_step (B) and the history - the position table (cases T N 2)
// when has_table, else cells (cases N Lcap), lengths (cases N), goal (cases N 2); out come the return code and x (B N 3 FOV+2
// FOV+2) as integers, one line each.  tests/test_host_semi_replay.py compares it with tests/semi_replay_restatement.py.
#include <cstdio>
#include <vector>

#include "../../magat_pathplanning_amd/csrc/magat_common.h"

int magat_prof_begin(int, hipStream_t) { return -1; }
void magat_prof_end(int, hipStream_t) {}
void magat_form_note(int) {}

#include "../../magat_pathplanning_amd/csrc/sim_guidance.hip"
#include "../../magat_pathplanning_amd/csrc/sim_guidance_wide.hip"

template <typename T>
static bool read_all(FILE* f, std::vector<T>& v) {
  for (auto& x : v) {
    long long t;
    if (fscanf(f, "%lld", &t) != 1) return false;
    x = (T)t;
  }
  return true;
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  int B, N, H, W, FOV, wide, has_table, cases, T, Lcap;
  if (!f || fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &B, &N, &H, &W, &FOV, &wide, &has_table, &cases, &T, &Lcap) != 10) return 2;
  if (B <= 0 || N <= 0 || H <= 0 || W <= 0 || FOV <= 0 || cases <= 0 || (has_table ? T <= 0 : Lcap <= 0)) return 2;
  std::vector<uint8_t> map((size_t)B * H * W);
  std::vector<int32_t> pos((size_t)B * N * 2), goal((size_t)B * N * 2), row_case(B), row_step(B);
  std::vector<int32_t> table(has_table ? (size_t)cases * T * N * 2 : 0), lengths(has_table ? 0 : (size_t)cases * N),
      hgoal(has_table ? 0 : (size_t)cases * N * 2);
  std::vector<uint16_t> cells(has_table ? 0 : (size_t)cases * N * Lcap);
  if (!read_all(f, map) || !read_all(f, pos) || !read_all(f, goal) || !read_all(f, row_case) || !read_all(f, row_step)) return 2;
  if (!read_all(f, table) || !read_all(f, cells) || !read_all(f, lengths) || !read_all(f, hgoal)) return 2;
  fclose(f);
  const int Wt = FOV + 2;
  std::vector<float> x((size_t)B * N * 3 * Wt * Wt, -7.f);
  magat_sim_history_desc h = {};
  h.row_case = row_case.data();
  h.row_step = row_step.data();
  h.cases = cases;
  if (has_table) {
    h.pos_table = table.data();
    h.T = T;
  } else {
    h.cells = cells.data();
    h.lengths = lengths.data();
    h.goal = hgoal.data();
    h.Lcap = Lcap;
  }
  int rc;
  if (wide) {
    const size_t bytes = magat_sim_guided_states_wide_workspace_bytes(B, N, H, W, FOV);
    std::vector<unsigned long long> ws(bytes / 8, 0xa5a5a5a5a5a5a5a5ull);      // exactly the size asked for
    rc = magat_sim_replayed_states_wide(map.data(), 1, H, W, pos.data(), goal.data(), x.data(), FOV, B, N, &h, ws.data(), bytes, nullptr);
  } else {
    rc = magat_sim_replayed_states(map.data(), 1, H, W, pos.data(), goal.data(), x.data(), FOV, B, N, &h, nullptr);
  }
  printf("%d\n", rc);
  for (size_t i = 0; i < x.size(); ++i) printf("%d%c", (int)x[i], i + 1 == x.size() ? '\n' : ' ');
  return 0;
}
