// pg_hof_scan.cpp -- DEAP's HallOfFame.update on the host (include/pong_ga.h):
// pg_hof_update, the general scan over (fitness, age) ranks, and
// pg_hof_update_packed, the generation's scan over the device's packed ranks
// and classes with the hall's slots assigned in place.  Plain C++17: no HIP
// header, compiled for the host alone (pong_amd/build.py).
#include <algorithm>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <vector>

#include "../../include/pong_ga.h"
#include "pg_fail.hpp"

using namespace pg;

extern "C" {

int32_t pg_hof_update(const pg_hof_args *a) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  if (a->maxsize < 0 || a->hof_n < 0 || a->hof_n > a->maxsize || a->pop_n < 0 || !a->new_n ||
      (a->maxsize > 0 && (!a->new_src || !a->new_fitness)) || (a->hof_n > 0 && (!a->hof_fitness || !a->hof_hash)) ||
      (a->pop_n > 0 && (!a->pop_fitness || !a->pop_hash)))
    return fail(PG_ERR_INVALID, "hof_update: bad sizes or NULL buffers");
  // Entries e < hof_n are the old members (items order), entries hof_n + i the
  // population.  Rank = position in ascending (fitness, age) order, age as
  // HallOfFame.keys orders equal fitness: later insertions rank higher.  The
  // hall is a presence bitmap over ranks; its worst member is the lowest
  // present rank, which only moves up while the hall is full (an entrant
  // beats the worst strictly), so each removal is an amortised O(1) scan.
  const int hn = a->hof_n, pn = a->pop_n, n = hn + pn;
  auto fit_of = [&](int e) { return e < hn ? a->hof_fitness[e] : a->pop_fitness[e - hn]; };
  auto hash_of = [&](int e) { return e < hn ? a->hof_hash[e] : a->pop_hash[e - hn]; };
  auto age_of = [&](int e) { return e < hn ? (hn - 1 - e) : e; };  // old member hn-1 is the oldest
  std::vector<int32_t> rank_v, by_rank((size_t)n);
  const int32_t *rank = a->rank;
  if (!rank) {
    std::vector<int32_t> order((size_t)n);
    for (int e = 0; e < n; ++e) order[e] = e;
    std::sort(order.begin(), order.end(), [&](int x, int y) {
      const double fx = fit_of(x), fy = fit_of(y);
      return fx < fy || (fx == fy && age_of(x) < age_of(y));
    });
    rank_v.resize((size_t)n);
    for (int r = 0; r < n; ++r) rank_v[order[r]] = r;
    rank = rank_v.data();
  }
  for (int e = 0; e < n; ++e) {
    if (rank[e] < 0 || rank[e] >= n) return fail(PG_ERR_INVALID, "hof_update: rank[%d]=%d out of range", e, rank[e]);
    by_rank[rank[e]] = e;
  }
  std::vector<uint64_t> present(((size_t)n + 63) / 64, 0);
  // Similarity classes: when every hash is a dense class id in [0, n) (DeviceGA
  // passes torch.unique's inverse), counts are a direct-indexed array; else a
  // flat open-addressing table keyed by the 64-bit row hash.
  bool dense = true;
  for (int e = 0; e < n && dense; ++e) dense = (uint64_t)hash_of(e) < (uint64_t)n;
  std::vector<int32_t> dense_count(dense ? (size_t)n : 0, 0);
  size_t cap = 1;
  if (!dense)
    while (cap < 2 * (size_t)n + 16) cap <<= 1;
  struct Slot {
    uint64_t key;
    int32_t count, used;
  };
  std::vector<Slot> table(dense ? 0 : cap, Slot{0, 0, 0});
  auto count_of = [&](uint64_t key) -> int32_t & {
    if (dense) return dense_count[key];
    size_t i = (size_t)(key * 0x9E3779B97F4A7C15ull) & (cap - 1);
    while (table[i].used && table[i].key != key) i = (i + 1) & (cap - 1);
    if (!table[i].used) table[i] = Slot{key, 0, 1};
    return table[i].count;
  };
  int size = 0, worst = n;  // lowest present rank (n: none)
  auto add = [&](int e) {
    const int r = rank[e];
    present[r >> 6] |= 1ull << (r & 63);
    count_of(hash_of(e)) += 1;
    size += 1;
    worst = r < worst ? r : worst;
  };
  for (int e = 0; e < hn; ++e) add(e);
  for (int i = 0; i < pn; ++i) {
    if (size == 0 && a->maxsize != 0) {  // DEAP: an empty hall takes population[0]
      add(hn);
      continue;
    }
    if (a->maxsize == 0) continue;
    const double f = a->pop_fitness[i];
    if (size >= a->maxsize && !(f > fit_of(by_rank[worst]))) continue;  // ind.fitness > self[-1].fitness
    if (count_of(a->pop_hash[i]) > 0) continue;                        // similar to a member
    if (size >= a->maxsize) {  // remove(-1): the worst, oldest among equal fitness
      present[worst >> 6] &= ~(1ull << (worst & 63));
      count_of(hash_of(by_rank[worst])) -= 1;
      size -= 1;
      size_t wd = (size_t)worst >> 6;
      uint64_t bits = present[wd] & (~0ull << (worst & 63));
      while (!bits && ++wd < present.size()) bits = present[wd];
      worst = bits ? (int)(wd * 64 + __builtin_ctzll(bits)) : n;
    }
    add(hn + i);
  }
  // items order: best first, newest first among equal fitness = descending rank
  int j = 0;
  for (size_t wd = present.size(); wd-- > 0;) {
    uint64_t bits = present[wd];
    while (bits) {
      const int hi = 63 - __builtin_clzll(bits);
      bits &= ~(1ull << hi);
      const int e = by_rank[wd * 64 + hi];
      a->new_src[j] = e;
      a->new_fitness[j] = fit_of(e);
      ++j;
    }
  }
  *a->new_n = j;
  return PG_OK;
}

namespace {
// The hall in place (pg_hof_packed_args.slot_out), for the general scan's
// result: kept members keep their slots; entering candidates take the freed
// slots -- those of the members not kept, in items order, then hof_n,
// hof_n + 1, ... -- in output order (the packed scan does the same inline).
int32_t assign_slots(int hn, int new_n, const int32_t *slot_in, const int32_t *src, int32_t *slot_out) {
  const auto slot_of = [&](int e) { return slot_in ? slot_in[e] : e; };
  std::vector<int32_t> freed;
  std::vector<uint8_t> kept((size_t)hn, 0);
  for (int j = 0; j < new_n; ++j)
    if (src[j] < hn) kept[src[j]] = 1;
  for (int e = 0; e < hn; ++e)
    if (!kept[e]) freed.push_back(slot_of(e));
  size_t next = 0;
  int grow = hn;
  for (int j = 0; j < new_n; ++j) {
    if (src[j] < hn) {
      slot_out[j] = slot_of(src[j]);
    } else if (next < freed.size()) {
      slot_out[j] = freed[next++];
    } else {
      slot_out[j] = grow++;
    }
  }
  if (grow > new_n) return fail(PG_ERR_INVALID, "hof_update_packed: slots beyond the new hall (%d > %d)", grow, new_n);
  return PG_OK;
}
}  // namespace

int32_t pg_hof_update_packed(const pg_hof_packed_args *a) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  const int hn = a->hof_n, k = a->k;
  if (a->maxsize < 0 || hn < 0 || hn > a->maxsize || k < 0 || !a->new_n || (a->maxsize > 0 && (!a->new_src || !a->new_fitness)) ||
      (hn > 0 && !a->hof_fitness) || (hn + k > 0 && !a->packed))
    return fail(PG_ERR_INVALID, "hof_update_packed: bad sizes or NULL buffers");
  if (a->slot_in && hn > 0) {  // (a min/max pass the compiler vectorises: the scan is on the generation's path)
    int32_t lo = a->slot_in[0], hi = a->slot_in[0];
    for (int e = 1; e < hn; ++e) {
      lo = a->slot_in[e] < lo ? a->slot_in[e] : lo;
      hi = a->slot_in[e] > hi ? a->slot_in[e] : hi;
    }
    if (lo < 0 || hi >= hn) return fail(PG_ERR_INVALID, "hof_update_packed: slot_in outside [0, hof_n) (%d..%d)", lo, hi);
  }
  const int64_t *pk = a->packed;
  const int n = hn + k;
  auto rank_of = [&](int e) { return (int32_t)(uint32_t)pk[e]; };
  auto class_of = [&](int e) { return (int32_t)(pk[e] >> 32); };
  auto cand_fit = [&](int c) {
    double f;
    std::memcpy(&f, &pk[n + c], sizeof(double));
    return f;
  };
  // the general scan: the packing decoded (an empty hall's first entrant, or
  // members whose ranks are not descending)
  const auto general = [&]() -> int32_t {
    std::vector<int32_t> rank((size_t)n);
    std::vector<uint64_t> hh((size_t)hn), ph((size_t)k);
    std::vector<double> pf((size_t)k);
    for (int e = 0; e < n; ++e) {
      rank[e] = rank_of(e);
      if (e < hn) hh[e] = (uint64_t)class_of(e);
      else ph[e - hn] = (uint64_t)class_of(e);
    }
    for (int c = 0; c < k; ++c) pf[c] = cand_fit(c);
    pg_hof_args g;
    g.maxsize = a->maxsize;
    g.hof_n = hn;
    g.hof_fitness = a->hof_fitness;
    g.hof_hash = hh.data();
    g.pop_n = k;
    g.pop_fitness = pf.data();
    g.pop_hash = ph.data();
    g.rank = rank.data();
    g.new_n = a->new_n;
    g.new_src = a->new_src;
    g.new_fitness = a->new_fitness;
    const int32_t rc = pg_hof_update(&g);
    if (rc != PG_OK || !a->slot_out) return rc;
    return assign_slots(hn, *a->new_n, a->slot_in, a->new_src, a->slot_out);
  };
  if (a->maxsize == 0) {
    *a->new_n = 0;
    return PG_OK;
  }
  if (hn == 0) return general();
  for (int e = 1; e < hn; ++e)
    if (rank_of(e) >= rank_of(e - 1)) return general();  // members not in items order
  for (int c = 0; c < k; ++c)
    if (class_of(hn + c) < 0 || class_of(hn + c) >= n) return fail(PG_ERR_INVALID, "hof_update_packed: class out of range");
  // accepted candidates present in the hall: a bitmap over the entries'
  // ranks (cmin = its lowest set bit) and rank -> candidate; their classes'
  // counts (candidate classes are >= hn)
  std::vector<uint64_t> cbits(((size_t)n + 63) / 64, 0);
  std::unique_ptr<int32_t[]> cand_at(new int32_t[(size_t)n]);  // read only where a bit is set
  int cmin = n;
  std::vector<int32_t> ccount((size_t)k, 0);
  // accepted candidates whose class is a member's (their row equals a member
  // evicted before them): rare, so a small map instead of an array of hof_n
  std::unordered_map<int32_t, int32_t> mcount;
  int p = hn - 1;  // members 0..p present: eviction takes the tail first
  int size = hn;
  for (int c = 0; c < k; ++c) {
    const double f = cand_fit(c);
    const int cls = class_of(hn + c);
    // the worst present entry: the tail member or the lowest-ranked accepted candidate
    const bool cand_worst = cmin < n && (p < 0 || cmin < rank_of(p));
    if (size >= a->maxsize) {  // ind.fitness > self[-1].fitness
      const double fw = cand_worst ? cand_fit(cand_at[cmin]) : a->hof_fitness[p];
      if (!(f > fw)) continue;
    }
    if (cls < hn ? (cls <= p || mcount.count(cls) > 0) : ccount[cls - hn] > 0) continue;  // similar to a present entry
    if (size >= a->maxsize) {  // remove(-1)
      if (cand_worst) {
        const int wc = class_of(hn + cand_at[cmin]);
        if (wc >= hn) {
          ccount[wc - hn] -= 1;
        } else if (--mcount[wc] == 0) {
          mcount.erase(wc);
        }
        cbits[(size_t)cmin >> 6] &= ~(1ull << (cmin & 63));
        size_t wd = (size_t)cmin >> 6;
        uint64_t bits = cbits[wd];
        while (!bits && ++wd < cbits.size()) bits = cbits[wd];
        cmin = bits ? (int)(wd * 64 + __builtin_ctzll(bits)) : n;
      } else {
        p -= 1;
      }
      size -= 1;
    }
    const int r = rank_of(hn + c);
    cbits[(size_t)r >> 6] |= 1ull << (r & 63);
    cand_at[r] = c;
    cmin = r < cmin ? r : cmin;
    if (cls >= hn) ccount[cls - hn] += 1;
    else mcount[cls] += 1;
    size += 1;
  }
  // items order: members 0..p (descending rank) merged with the present
  // candidates by descending rank (the bitmap walked down), member runs
  // copied as ranges
  // (slot_out: a member run keeps its slots; a candidate takes the next freed
  // slot -- the evicted tail p+1..hn-1's, then hn, hn + 1, ...)
  int32_t *so = a->slot_out;
  int freed = p + 1, grow = hn;
  const auto member_run = [&](int j0, int from, int to) {
    for (int e = from; e < to; ++e) a->new_src[j0 + e - from] = e;
    std::memcpy(a->new_fitness + j0, a->hof_fitness + from, sizeof(double) * (size_t)(to - from));
    if (so) {
      if (a->slot_in) std::memcpy(so + j0, a->slot_in + from, sizeof(int32_t) * (size_t)(to - from));
      else
        for (int e = from; e < to; ++e) so[j0 + e - from] = e;
    }
  };
  int j = 0, m = 0;  // output position, next member
  for (size_t wd = cbits.size(); wd-- > 0;) {
    uint64_t bits = cbits[wd];
    while (bits) {
      const int hi = 63 - __builtin_clzll(bits);
      bits &= ~(1ull << hi);
      const int r = (int)(wd * 64 + hi), c = cand_at[r];
      int lo = m;  // the members ranked above this candidate
      while (lo <= p && rank_of(lo) > r) ++lo;
      member_run(j, m, lo);
      j += lo - m;
      m = lo;
      a->new_src[j] = hn + c;
      a->new_fitness[j] = cand_fit(c);
      if (so) so[j] = freed < hn ? (a->slot_in ? a->slot_in[freed++] : freed++) : grow++;
      ++j;
    }
  }
  if (p + 1 > m) member_run(j, m, p + 1);
  j += p + 1 > m ? p + 1 - m : 0;
  *a->new_n = j;
  if (so && grow > j) return fail(PG_ERR_INVALID, "hof_update_packed: slots beyond the new hall (%d > %d)", grow, j);
  return PG_OK;
}

}  // extern "C"
