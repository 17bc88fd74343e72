// The schedule improver of both map widths - sim_mapf_lns.hip and sim_mapf_lns_wide.hip - once: neighbourhood re-planning on top of
// prioritized planning (MAPF-LNS; DESIGN 4.11, restated cell by cell in tests/lns_restatement.py).  It is NOT ECBS: no bound on the
// flowtime - the only promises are that the flowtime never rises and that a valid schedule stays valid.  One workgroup per case runs
// mapf_lns_walk; the kernel carves the workspace and hands in a form, which brings what differs between the two:
//   the group               sim_group.h: tid, nt, the free board, the reductions and counts behind a barrier of the workgroup
//   clear_boards            the reservation boards of every t zeroed (an R layer is written before it is read)
//   board_word(t, b, r, c)  the word of board b of layer t that holds cell (r, c); its bit there is c & 63
//   stage_old(nb, m, rows, len, T), old(j, row)   the old paths of the neighbourhood: staged in LDS, behind a barrier of the form's
//                           own, and read from there (narrow), or read from their global rows (wide)
//   search<BOARDS>, trace<BOARDS>   the low-level search of one agent and its backtrace, the planner's own (sim_mapf_parts.h,
//                           sim_mapf_wide_parts.h); BOARDS = false compiles the board loads out: an agent's FREE path.  What a form
//                           needs between its search and its trace is the form's (narrow: a barrier; wide: the search's last round)
// Integer and bit arithmetic only, no random numbers.  Per case, on a solved schedule (an agent's cell at t: paths[a][min(t, length - 1)]):
//   screening      solved == 0: status 1; a length outside 1..T, one of the T cells of a row off the map or on an obstacle, a
//                  step that is none of the five moves: status 2.  Such a case is left as it came.  Threads over t.
//   set-up         all N paths reserved (each staged in LDS first), threads over t: layer t belongs to one thread; d0[a] = the
//                  length of a's free path.
//   iteration i    seed = the (i mod N)-th agent by (-delay, index), delay = length - d0: found by counting, threads over agents in
//                  chunks of nt - a bisection over the delay, then the index inside the class (a thread's place is what group_count
//                  puts in front of it), written to one LDS int.  The seed's free path is searched and traced again; along it the
//                  agents standing on its cell at t or swapping with it join the neighbourhood: a newcomer takes the place m +
//                  `before` behind the list, so they come in index order across waves and chunks, at most k; then seed + 1, seed +
//                  2, ...  The OLD paths of the neighbourhood are staged in LDS (narrow) or read from `paths` (wide) - the
//                  global rows are overwritten only on accept -, un-reserved, its agents re-planned in list order and reserved,
//                  the NEW paths staged in LDS; accepted iff everybody arrived and the lengths sum to strictly less - only then
//                  are the global paths and lengths overwritten - else the new paths are cleared and the old ones reserved again
//                  (exact: in a valid schedule no two agents share a V or an A_d bit).
// The barriers: the union of what the two kernels had, but for the two that only the narrow layout needs (search | trace, staged old
// cells | un-reserve) - those stand in the narrow form's hooks, where a barrier of one wavefront costs nothing, and the wide form keeps
// the sequence of rounds it had.  What each protects:
//   after publish_free      the free rows are read by other threads;  after clear_boards: the boards are marked by other threads
//   set-up: staged | marked, and the end of an agent: the staged path is read by other threads and staged again; d0
//   top of an iteration     d0, and the lengths and paths of an accepted iteration; the seed slot is set to -1 behind it
//   seed slot | read        the slot is written by the thread that found itself (behind group_count's barrier), read by everybody
//   trace | scan            fcells and nb[0] are read by other threads
//   group_count | nb write | next read     every thread has read nb before a newcomer is written, and sees it afterwards
//   fill-up                 the same, around thread 0's write
//   un-reserve | search, trace | mark | next search     every load of the boards lies behind the marks; old_len, new_cells and
//                           new_len are read by other threads
//   roll back               new paths cleared | old paths reserved;  before the closing reduction: the lengths of the last accept
// Every branch around a barrier or a group_* call is uniform over the workgroup: its condition comes out of a group reduction or
// is read from one address by all threads.  Every store is a per-thread (vector) store from plain C++.
#pragma once
#include <cstdint>

#include "magat_common.h"
#include "sim_entry.h"      // sim_entry_check
#include "sim_group.h"

constexpr int LNS_MAX_K = 8;
constexpr int LNS_MAX_ITERATIONS = 4096;

// what the walk keeps in LDS, MAX_T the form's horizon
template <int MAX_T>
struct lns_stage {
  int fcells[MAX_T];                    // the seed's free path
  int new_cells[LNS_MAX_K][MAX_T];      // the re-planned paths
  int nb[LNS_MAX_K], old_len[LNS_MAX_K], new_len[LNS_MAX_K];      // (old_len: a length out of LDS spares the re-plan a round of global loads)
  int seed;
};
// one case: its slices of the inputs, and of the workspace and LDS what the walk itself reads and writes
struct lns_case {
  const uint8_t* map;
  int H, W, solved;
  int *rows, *len;      // `paths` and `lengths`; agent a's row: rows + a * T * 2
  int* d0;
  u64* free_rows;       // LDS, for publish_free
  int N, T;
};
struct lns_out {
  int *makespan, *flow_before, *flow_after, *accepted, *status;
};

// a global path row as cells (row << 8 | col), and a staged one
struct lns_row {
  const int* p;
  __device__ __forceinline__ int operator()(int t) const { return p[2 * t] << 8 | p[2 * t + 1]; }
};
struct lns_staged {
  const int* cells;
  __device__ __forceinline__ int operator()(int t) const { return cells[t]; }
};

// Reserves (SET) or un-reserves one path, threads over t: layer t belongs to one thread, so no two threads touch one word.
// cell(t), 0 <= t < len: the path's cell.  V[t] along the path and at its last cell behind it, A_d[t] at the entered cell of a
// real move.
template <bool SET, class Form, class Cell>
__device__ __forceinline__ void lns_mark(Form& f, Cell cell, int len, int T) {
  for (int t = f.tid; t < T; t += f.nt) {
    const int at = cell(t < len ? t : len - 1), cr = at >> 8, cc = at & 255;
    u64* v = f.board_word(t, 0, cr, cc);
    if (SET) *v |= 1ull << (cc & 63);
    else *v &= ~(1ull << (cc & 63));
    if (t >= 1 && t < len) {
      const int from = cell(t - 1), dr = cr - (from >> 8), dc = cc - (from & 255);
      const int d = dr == -1 ? 0 : dc == -1 ? 1 : dr == 1 ? 2 : dc == 1 ? 3 : 4;
      if (d < 4) {
        u64* a = f.board_word(t, 1 + d, cr, cc);
        if (SET) *a |= 1ull << (cc & 63);
        else *a &= ~(1ull << (cc & 63));
      }
    }
  }
}

// how many agents have delay = length - d0 >= x (the same for every thread): a ballot per chunk, one round across the waves
template <class Form>
__device__ __forceinline__ int lns_count_ge(Form& f, const int* len, const int* d0, int N, int x) {
  int cnt = 0;
  for (int base = 0; base < N; base += f.nt) {
    const int b = base + f.tid;
    cnt += __popcll(__builtin_amdgcn_ballot_w64(b < N && len[b < N ? b : 0] - d0[b < N ? b : 0] >= x));
  }
  return f.group_sum_waves(cnt);
}

// (always inlined: the form is then the kernel's own local and dissolves into registers)
template <class Form, int MAX_T>
__device__ __forceinline__ void mapf_lns_walk(Form& f, const lns_case& k, lns_stage<MAX_T>& lds, const lns_out& out, int cs,
                                              int iterations, int K) {
  const int tid = f.tid, nt = f.nt, N = k.N, T = k.T, H = k.H, W = k.W;
  int *rows = k.rows, *len = k.len, *d0 = k.d0, *nb = lds.nb;
  if (tid == 0) {
    out.flow_before[cs] = 0;
    out.flow_after[cs] = 0;
    out.accepted[cs] = 0;
  }
  if (k.solved == 0) {
    if (tid == 0) out.status[cs] = 1;
    return;
  }
  f.load_free(k.map, H, W);
  f.publish_free(k.free_rows);
  __syncthreads();
  // screening, threads over t
  bool bad = false;
  for (int a = 0; a < N; ++a) {
    const int la = len[a];
    bad |= la < 1 || la > T;
    const int* p = rows + (long long)a * T * 2;
    for (int t = tid; t < T; t += nt) {
      const int r = p[2 * t], c = p[2 * t + 1];
      const bool inside = r >= 0 && r < H && c >= 0 && c < W;
      bad |= !inside || !f.is_free(inside ? r : 0, inside ? c : 0);
      if (t >= 1 && inside) {
        const int pr = p[2 * t - 2], pc = p[2 * t - 1];
        const bool pin = pr >= 0 && pr < H && pc >= 0 && pc < W;      // (a cell outside is refused by its own thread)
        const int dr = pin ? r - pr : 0, dc = pin ? c - pc : 0;
        bad |= !((dr == 0 && dc >= -1 && dc <= 1) || (dc == 0 && dr >= -1 && dr <= 1));
      }
    }
  }
  if (f.group_or((int)bad)) {
    if (tid == 0) out.status[cs] = 2;
    return;
  }
  // set-up: every path reserved, d0 of every agent, the flowtime
  f.clear_boards();
  __syncthreads();
  int flow = 0;
  for (int a = 0; a < N; ++a) {
    const int la = __builtin_amdgcn_readfirstlane(len[a]);
    const lns_row row{rows + (long long)a * T * 2};
    int* cells = lds.new_cells[0];      // staged: ONE round of global loads per agent, then LDS
    for (int t = tid; t < la; t += nt) cells[t] = row(t);
    __syncthreads();
    lns_mark<true>(f, lns_staged{cells}, la, T);
    const int s = __builtin_amdgcn_readfirstlane(cells[0]), g = __builtin_amdgcn_readfirstlane(cells[la - 1]);
    const int tfree = f.template search<false>(s >> 8, s & 255, g >> 8, g & 255);
    if (tid == 0) d0[a] = tfree < 0 ? la : tfree + 1;      // (the path itself is a witness: tfree <= la - 1)
    flow += la - 1;
    __syncthreads();      // the path is staged again
  }
  if (tid == 0) out.flow_before[cs] = flow;
  const int kk = K < N ? K : N;
  int taken = 0;
  for (int it = 0; it < iterations; ++it) {
    __syncthreads();      // d0, and the lengths and paths of an accepted iteration
    if (tid == 0) lds.seed = -1;      // (set again behind the first barrier of the chunk loop below)
    // the seed: the (it mod N)-th agent by (-delay, index); 0 <= delay < T
    const int rank = it % N;
    int lo = 0, hi = T, above = 0;      // count(delay >= lo) > rank >= count(delay >= hi) = above
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1, cnt = lns_count_ge(f, len, d0, N, mid);
      if (cnt > rank) lo = mid;
      else hi = mid, above = cnt;
    }
    for (int base = 0, seen = above; base < N && seen <= rank; base += nt) {      // the (rank - above)-th agent, in index order, with delay == lo
      const int b = base + tid;
      const bool in_class = b < N && len[b < N ? b : 0] - d0[b < N ? b : 0] == lo;
      int before = 0;
      const int members = f.group_count(in_class, &before);
      if (in_class && seen + before == rank) lds.seed = b;
      seen += members;
    }
    __syncthreads();
    const int seed = lds.seed;
    if (seed < 0 || seed >= N) continue;      // (cannot happen: every delay lies in 0 .. T - 1)
    // the seed's free path
    const int ls = __builtin_amdgcn_readfirstlane(len[seed]);
    const int* ps = rows + (long long)seed * T * 2;
    const int sr = __builtin_amdgcn_readfirstlane(ps[0]), sc = __builtin_amdgcn_readfirstlane(ps[1]);
    const int gr = __builtin_amdgcn_readfirstlane(ps[2 * ls - 2]), gc = __builtin_amdgcn_readfirstlane(ps[2 * ls - 1]);
    const int tfree = f.template search<false>(sr, sc, gr, gc);
    if (tfree < 0) continue;                  // (cannot happen either)
    f.template trace<false>(lds.fcells, gr, gc, tfree);
    if (tid == 0) nb[0] = seed;
    __syncthreads();
    // the neighbourhood: who is in the way of the free path, threads over agents
    int m = 1;
    for (int t = 0; t <= tfree && m < kk; ++t) {
      const int fc = lds.fcells[t], fp = t >= 1 ? lds.fcells[t - 1] : -1;
      for (int base = 0; base < N && m < kk; base += nt) {
        const int b = base + tid;
        bool in = false;
        if (b < N) {
          const int lb = len[b];
          const lns_row pb{rows + (long long)b * T * 2};
          const int cb = pb(t < lb ? t : lb - 1);
          in = cb == fc;
          if (!in && t >= 1 && cb == fp) in = pb(t - 1 < lb ? t - 1 : lb - 1) == fc;
          for (int j = 0; j < m; ++j) in = in && nb[j] != b;
        }
        int before = 0;
        const int total = f.group_count(in, &before);      // (its barrier: every thread has read nb)
        if (total) {      // newcomers in index order
          if (in && m + before < kk) nb[m + before] = b;
          m = m + total < kk ? m + total : kk;
          __syncthreads();
        }
      }
    }
    for (int step = 1; m < kk && step < N; ++step) {      // fill up with seed + 1, seed + 2, ...
      const int b = (seed + step) % N;
      bool in = false;
      for (int j = 0; j < m; ++j) in = in || nb[j] == b;
      if (!in) {
        __syncthreads();
        if (tid == 0) nb[m] = b;
        ++m;
        __syncthreads();
      }
    }
    // un-reserve the old paths: read where the form keeps them - its stage, or their global rows
    int old_sum = 0;
    for (int j = 0; j < m; ++j) {
      const int la = __builtin_amdgcn_readfirstlane(len[nb[j]]);
      if (tid == 0) lds.old_len[j] = la;
      old_sum += la;
    }
    f.stage_old(nb, m, rows, len, T);
    for (int j = 0; j < m; ++j)
      lns_mark<false>(f, f.old(j, lns_row{rows + (long long)nb[j] * T * 2}), __builtin_amdgcn_readfirstlane(len[nb[j]]), T);
    __syncthreads();
    // re-plan in list order, each agent against everything reserved now
    int done = 0, new_sum = 0;
    for (; done < m; ++done) {
      const auto old = f.old(done, lns_row{rows + (long long)nb[done] * T * 2});
      const int la = lds.old_len[done];
      const int s = __builtin_amdgcn_readfirstlane(old(0)), g = __builtin_amdgcn_readfirstlane(old(la - 1));
      const int tstar = f.template search<true>(s >> 8, s & 255, g >> 8, g & 255);
      if (tstar < 0) break;
      f.template trace<true>(lds.new_cells[done], g >> 8, g & 255, tstar);
      if (tid == 0) lds.new_len[done] = tstar + 1;
      __syncthreads();
      lns_mark<true>(f, lns_staged{lds.new_cells[done]}, tstar + 1, T);
      new_sum += tstar + 1;
      __syncthreads();      // the next agent loads these boards
    }
    if (done == m && new_sum < old_sum) {
      for (int j = 0; j < m; ++j) {
        const int a = nb[j], ln = lds.new_len[j];
        int* p = rows + (long long)a * T * 2;
        for (int t = tid; t < T; t += nt) {
          const int cell = lds.new_cells[j][t < ln ? t : ln - 1];
          p[2 * t] = cell >> 8;
          p[2 * t + 1] = cell & 255;
        }
        if (tid == 0) len[a] = ln;
      }
      ++taken;
    } else {
      for (int j = 0; j < done; ++j) lns_mark<false>(f, lns_staged{lds.new_cells[j]}, lds.new_len[j], T);
      __syncthreads();
      for (int j = 0; j < m; ++j) lns_mark<true>(f, f.old(j, lns_row{rows + (long long)nb[j] * T * 2}), lds.old_len[j], T);
    }
  }
  __syncthreads();
  int total = 0, longest = 1;
  for (int b = tid; b < N; b += nt) {
    total += len[b] - 1;
    longest = len[b] > longest ? len[b] : longest;
  }
  total = f.group_sum(total);      // (two rounds, not one group_sum_max: with it the wide form's 65 x 65 row measured 1.8 % slower,
  longest = f.group_max(longest);  // against 0.3 % - profiles/mapf_walks/latency.txt, below the table)
  if (tid == 0) {
    out.makespan[cs] = longest - 1;
    out.flow_after[cs] = total;
    out.accepted[cs] = taken;
    out.status[cs] = 0;
  }
}

// what the two entries refuse alike, in the ladder's order (sim_entry.h); an entry brings its map side, horizon and bytes
inline int lns_entry_check(std::initializer_list<const void*> pointers, int H, int W, int C, int N, int T, int iterations, int k,
                           int side, int max_t, const void* workspace, size_t workspace_bytes, size_t need) {
  return sim_entry_check(pointers, H > 0 && W > 0 && C > 0 && N > 0 && T > 0,
                         H <= side && W <= side && T <= max_t && k >= 1 && k <= LNS_MAX_K && iterations >= 0 && iterations <= LNS_MAX_ITERATIONS,
                         workspace, workspace_bytes, need);
}
