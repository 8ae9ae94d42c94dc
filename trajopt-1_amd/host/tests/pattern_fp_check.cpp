// The workgroup sparsity fingerprint (csrc/pattern_fp.hpp, sqp_kernel.hip
// pattern_fingerprint_wg) replayed "thread by thread" on the host and compared,
// as an equal / not-equal decision between two QP set-ups, with
//   * the literal test of OSQPModel (quirk Q2): n, m and nnz equal and a memcmp
//     of the first n + 1 bytes of the int64 column pointers and the first nnz
//     bytes of the int64 row indices of A in CSC form, and
//   * a transcription of the serial walk (sqp_kernel.hip pattern_fingerprint).
// Random pairs first, then pairs built so that exactly one compared element
// (or one just past a prefix, or the bytes above the compared ones of the
// partial last element) differs, whose decision is known beforehand.
// Own main, no GPU call; built with the sanitizers by `make san-patternfp`.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../csrc/pattern_fp.hpp"

using thip::FpDims;
using thip::FpPrefix;

namespace
{
constexpr int kThreads = 256;  // layout.hpp kBlock

struct Pattern
{
  int D = 7, N = 0, n_abs = 0, nh = 0, hinge = 1;
  std::vector<int> fos, step_ptr, step_rows, row_step, mask, HP, HM;
  int n_fixed_rows = 0;
  int nx() const { return D * N; }
  int n_rows() const { return n_fixed_rows + n_abs; }
  int nc_base() const { return nx() + 2 * n_abs; }
  int n() const { return nc_base() + nh; }
  int m() const { return n_rows() + nh + n(); }
  FpDims dims() const
  {
    FpDims d;
    d.D = D;
    d.N = N;
    d.nx = nx();
    d.nc_base = nc_base();
    d.n_fixed_rows = n_fixed_rows;
    d.n_rows = n_rows();
    d.nh = nh;
    d.hinge = hinge;
    return d;
  }
};

// rows_per_step abs rows at every waypoint, nh hinge rows dealt over the step pairs
Pattern make_pattern(std::mt19937_64& rng, int D, int N, int rows_per_step, int nh, int hinge, double density)
{
  Pattern p;
  p.D = D;
  p.N = N;
  p.hinge = hinge;
  p.nh = hinge ? nh : 0;
  std::uniform_real_distribution<double> u(0.0, 1.0);
  p.fos.assign(N, -1);
  int nf = 0;
  for (int t = 0; t < N; ++t)
    if (t == 0 || u(rng) < 0.1)
      p.fos[t] = nf++;
  p.n_fixed_rows = nf * D;
  p.step_ptr.assign(N + 1, 0);
  for (int t = 0; t < N; ++t)
  {
    const int nr = (rows_per_step > 0 && u(rng) < 0.15) ? rows_per_step + 5 : rows_per_step;  // some above 8: two groups
    for (int k = 0; k < nr; ++k)
    {
      p.step_rows.push_back(p.n_abs);
      p.row_step.push_back(t);
      int mk = 0;
      for (int j = 0; j < D; ++j)
        mk |= (u(rng) < density) << j;
      p.mask.push_back(mk);
      ++p.n_abs;
    }
    p.step_ptr[t + 1] = p.n_abs;
  }
  // hinge rows by step pair 0 .. N - 2 (HP[t] the first row of pair t; HP[N - 1] = HP[N] = nh)
  std::vector<int> per(N > 1 ? N - 1 : 1, 0);
  for (int h = 0; h < p.nh; ++h)
    per[static_cast<size_t>(u(rng) * u(rng) * per.size()) % per.size()]++;  // early pairs heavier
  p.HP.assign(N + 1, 0);
  for (int t = 0; t + 1 < N; ++t)
    p.HP[t + 1] = p.HP[t] + per[t];
  p.HP[N] = p.HP[N - 1];
  for (int h = 0; h < p.nh; ++h)
  {
    int mk = 0;
    for (int e = 0; e < 2 * D; ++e)
      mk |= (u(rng) < density) << e;
    p.HM.push_back(mk);
  }
  if (p.HM.empty())
    p.HM.push_back(0);  // the workspace array exists without rows
  return p;
}

// A in CSC form from the matrix itself: the set of rows of every column
void build_csc(const Pattern& p, std::vector<int64_t>& cp, std::vector<int64_t>& ci)
{
  const int D = p.D, nx = p.nx(), n = p.n();
  const int64_t row_hinge0 = p.n_rows(), row_ident0 = p.n_rows() + p.nh;
  std::vector<std::set<int64_t>> cols(n);
  for (int t = 0; t < p.N; ++t)
    if (p.fos[t] >= 0)
      for (int j = 0; j < D; ++j)
        cols[t * D + j].insert(static_cast<int64_t>(p.fos[t]) * D + j);
  for (int r = 0; r < p.n_abs; ++r)
  {
    for (int j = 0; j < D; ++j)
      if ((p.mask[r] >> j) & 1)
        cols[p.row_step[r] * D + j].insert(p.n_fixed_rows + r);
    cols[nx + 2 * r].insert(p.n_fixed_rows + r);
    cols[nx + 2 * r + 1].insert(p.n_fixed_rows + r);
  }
  if (p.hinge)
    for (int t = 0; t + 1 < p.N; ++t)
      for (int h = p.HP[t]; h < p.HP[t + 1]; ++h)
        for (int e = 0; e < 2 * D; ++e)
          if ((p.HM[h] >> e) & 1)
            cols[(t + e / D) * D + e % D].insert(row_hinge0 + h);
  for (int h = 0; h < p.nh; ++h)
    cols[p.nc_base() + h].insert(row_hinge0 + h);
  for (int col = 0; col < n; ++col)
    cols[col].insert(row_ident0 + col);
  cp.assign(1, 0);
  ci.clear();
  for (int col = 0; col < n; ++col)
  {
    ci.insert(ci.end(), cols[col].begin(), cols[col].end());
    cp.push_back(static_cast<int64_t>(ci.size()));
  }
}

struct Fp
{
  unsigned long long hash;
  int n, m;
  long long nnz;
  bool operator==(const Fp& o) const { return hash == o.hash && n == o.n && m == o.m && nnz == o.nnz; }
};

// pattern_fingerprint_wg, one thread after the other between its barriers
Fp fingerprint_wg(const Pattern& p)
{
  const FpDims d = p.dims();
  const int nx = d.nx, n = d.n();
  const int *fos = p.fos.data(), *sp = p.step_ptr.data(), *sr = p.step_rows.data(), *mask = p.mask.data(),
            *HP = p.HP.data(), *HM = p.HM.data();
  long long bits = 0;
  for (int tid = 0; tid < kThreads; ++tid)
  {
    for (int r = tid; r < p.n_abs; r += kThreads)
      bits += thip::fp_popc(mask[r]);
    for (int h = tid; h < p.nh; h += kThreads)
      bits += thip::fp_popc(HM[h]);
  }
  const long long nnz = thip::fp_nnz(d, p.n_abs, bits);
  const FpPrefix P = thip::fp_prefix(n, nnz);
  unsigned long long acc = 0;
  long long base_e = 0;
  int c0 = 0;
  do
  {
    std::vector<int> cnt(kThreads, 0);
    const FpPrefix unset = thip::fp_prefix(n, 0);
    for (int tid = 0; tid < kThreads; ++tid)
    {
      unsigned long long none = 0;
      const int col = c0 + tid;
      if (col < nx)
        cnt[tid] = thip::fp_x_column<false>(d, fos, sp, sr, mask, HP, HM, col, unset, 0, none);
    }
    long long run = base_e;  // the exclusive scan
    for (int tid = 0; tid < kThreads; ++tid)
    {
      const int col = c0 + tid;
      if (col < nx)
      {
        acc += thip::fp_ptr_term(P, col, run);
        thip::fp_x_column<true>(d, fos, sp, sr, mask, HP, HM, col, P, run, acc);
      }
      run += cnt[tid];
    }
    base_e = run;
    c0 += kThreads;
  } while (c0 < nx);
  const int last = thip::fp_tail_last(d, P, base_e);
  for (int tid = 0; tid < kThreads; ++tid)
    for (int col = nx + tid; col <= last; col += kThreads)
      acc += thip::fp_tail_column(d, P, base_e, col);
  return Fp{0x6A09E667F3BCC908ULL + acc, n, p.m(), nnz};
}

// sqp_kernel.hip pattern_fingerprint, transcribed
unsigned long long serial_mix(unsigned long long h, unsigned long long v)
{
  h ^= v + 0x9E3779B97F4A7C15ULL + (h << 6) + (h >> 2);
  return h * 0xBF58476D1CE4E5B9ULL;
}

Fp fingerprint_serial(const Pattern& p)
{
  const int D = p.D, nx = p.nx(), nh = p.nh, n = p.n();
  long long nnz = static_cast<long long>(p.n_fixed_rows) + 2LL * p.n_abs + nh + n;
  for (int r = 0; r < p.n_abs; ++r)
    nnz += __builtin_popcount(static_cast<unsigned>(p.mask[r]));
  for (int h = 0; h < nh; ++h)
    nnz += __builtin_popcount(static_cast<unsigned>(p.HM[h]));
  const long long row_hinge0 = p.n_rows(), row_ident0 = static_cast<long long>(p.n_rows()) + nh;
  const long long kp = (n + 1) / 8, kpr = (n + 1) % 8, ki = nnz / 8, kir = nnz % 8;
  auto low = [](unsigned long long v, long long bytes) {
    return bytes >= 8 ? v : (v & ((1ULL << (8 * bytes)) - 1ULL));
  };
  unsigned long long h = 0x6A09E667F3BCC908ULL;
  long long ptr = 0, e = 0;
  auto entry = [&](long long row) {
    if (e < ki)
      h = serial_mix(h, static_cast<unsigned long long>(row));
    else if (e == ki && kir)
      h = serial_mix(h, low(static_cast<unsigned long long>(row), kir) ^ 0x5555ULL);
    ++e;
  };
  for (int col = 0; col <= n; ++col)
  {
    if (col < kp)
      h = serial_mix(h, static_cast<unsigned long long>(ptr));
    else if (col == kp && kpr)
      h = serial_mix(h, low(static_cast<unsigned long long>(ptr), kpr) ^ 0xAAAAULL);
    if (col == n || (col >= kp && e > ki))
      break;
    const long long e0 = e;
    if (col < nx)
    {
      const int t = col / D, j = col % D;
      if (p.fos[t] >= 0)
        entry(static_cast<long long>(p.fos[t]) * D + j);
      for (int q = p.step_ptr[t]; q < p.step_ptr[t + 1]; ++q)
      {
        const int r = p.step_rows[q];
        if ((p.mask[r] >> j) & 1)
          entry(p.n_fixed_rows + r);
      }
      if (p.hinge)
      {
        if (t > 0)
          for (int hh = p.HP[t - 1]; hh < p.HP[t]; ++hh)
            if ((p.HM[hh] >> (D + j)) & 1)
              entry(row_hinge0 + hh);
        if (t < p.N - 1)
          for (int hh = p.HP[t]; hh < p.HP[t + 1]; ++hh)
            if ((p.HM[hh] >> j) & 1)
              entry(row_hinge0 + hh);
      }
    }
    else if (col < p.nc_base())
      entry(p.n_fixed_rows + (col - nx) / 2);
    else
      entry(row_hinge0 + (col - p.nc_base()));
    entry(row_ident0 + col);
    ptr += e - e0;
  }
  return Fp{h, n, p.m(), nnz};
}

struct Tally
{
  int pairs = 0, equal = 0, bad = 0;
};

// one pair through the three tests, with a message when they disagree; returns the memcmp decision
bool check_pair(const std::string& what, const Pattern& a, const Pattern& b, Tally& t)
{
  std::vector<int64_t> pa, ia, pb, ib;
  build_csc(a, pa, ia);
  build_csc(b, pb, ib);
  const Fp wa = fingerprint_wg(a), wb = fingerprint_wg(b), sa = fingerprint_serial(a), sb = fingerprint_serial(b);
  bool ok = wa.nnz == static_cast<long long>(ia.size()) && wb.nnz == static_cast<long long>(ib.size());
  bool ref = a.n() == b.n() && a.m() == b.m() && ia.size() == ib.size();
  if (ref)
    ref = std::memcmp(pa.data(), pb.data(), static_cast<size_t>(a.n() + 1)) == 0 &&
          std::memcmp(ia.data(), ib.data(), ia.size()) == 0;
  const bool wg = wa == wb, serial = sa == sb;
  ok = ok && wg == ref && serial == ref;
  t.pairs++;
  t.equal += ref;
  if (!ok)
  {
    t.bad++;
    std::printf("FAIL %s: memcmp %d, workgroup %d, serial %d (n %d / %d, nnz %lld / %lld, CSC %zu / %zu)\n", what.c_str(),
                ref, wg, serial, a.n(), b.n(), wa.nnz, wb.nnz, ia.size(), ib.size());
  }
  return ref;
}

// the same, for a pair built so that the memcmp decision is known beforehand
void check_expect(const std::string& what, const Pattern& a, const Pattern& b, Tally& t, bool expect_equal)
{
  if (check_pair(what, a, b, t) != expect_equal)
  {
    t.bad++;
    std::printf("FAIL %s: built to compare %s, the memcmp says otherwise\n", what.c_str(),
                expect_equal ? "equal" : "unequal");
  }
}

// moves bit `from` of v to `to` (nnz unchanged); false if that is no change
bool move_bit(int& v, int from, int to)
{
  if (!((v >> from) & 1) || ((v >> to) & 1))
    return false;
  v = (v & ~(1 << from)) | (1 << to);
  return true;
}

// a mask bit of an abs row of waypoint t moved to another column
bool move_abs_bit(Pattern& p, int t, std::mt19937_64& rng)
{
  for (int q = p.step_ptr[t]; q < p.step_ptr[t + 1]; ++q)
    for (int tries = 0; tries < 20; ++tries)
      if (move_bit(p.mask[p.step_rows[q]], static_cast<int>(rng() % p.D), static_cast<int>(rng() % p.D)))
        return true;
  return false;
}

bool move_hinge_bit(Pattern& p, int h, std::mt19937_64& rng)
{
  for (int tries = 0; tries < 40; ++tries)
    if (move_bit(p.HM[h], static_cast<int>(rng() % (2 * p.D)), static_cast<int>(rng() % (2 * p.D))))
      return true;
  return false;
}

// ---- pairs built from the known prefix: one element changes, at a chosen distance from a prefix's end ----

long long nnz_of(const Pattern& p);
// the prefixes' extents from the byte counts themselves, not from the header under test
FpPrefix literal_prefix(int n, long long nnz) { return FpPrefix{(n + 1) / 8, (n + 1) % 8, nnz / 8, nnz % 8}; }

long long nnz_of(const Pattern& p)
{
  long long nnz = static_cast<long long>(p.n_fixed_rows) + 2LL * p.n_abs + p.nh + p.n();
  for (int r = 0; r < p.n_abs; ++r)
    nnz += __builtin_popcount(static_cast<unsigned>(p.mask[r]));
  for (int h = 0; h < p.nh; ++h)
    nnz += __builtin_popcount(static_cast<unsigned>(p.HM[h]));
  return nnz;
}

// Brings nnz to target by setting or clearing mask bits whose columns all belong to waypoints > t_last (the abs
// rows of those waypoints, the hinge rows of step pairs > t_last), so no entry of an earlier column moves
bool tune_nnz(Pattern& p, int t_last, long long target)
{
  long long nnz = nnz_of(p);
  auto step = [&](int& v, int bit) {
    const bool on = (v >> bit) & 1;
    if (nnz < target && !on)
      v |= 1 << bit, ++nnz;
    else if (nnz > target && on)
      v &= ~(1 << bit), --nnz;
  };
  for (int r = p.n_abs - 1; r >= 0 && nnz != target; --r)
    if (p.row_step[r] > t_last)
      for (int j = 0; j < p.D && nnz != target; ++j)
        step(p.mask[r], j);
  if (p.hinge)
    for (int t = p.N - 2; t > t_last && nnz != target; --t)
      for (int h = p.HP[t]; h < p.HP[t + 1] && nnz != target; ++h)
        for (int e = 0; e < 2 * p.D && nnz != target; ++e)
          step(p.HM[h], e);
  return nnz == target;
}

// number of the entry (col, row) of A, -1 if A has none
long long entry_of(const std::vector<int64_t>& cp, const std::vector<int64_t>& ci, int col, int64_t row)
{
  for (int64_t e = cp[col]; e < cp[col + 1]; ++e)
    if (ci[e] == row)
      return e;
  return -1;
}

// hinge rows per step pair replaced by per[] (random masks)
void set_hinge(Pattern& p, const std::vector<int>& per, std::mt19937_64& rng, double density)
{
  std::uniform_real_distribution<double> u(0.0, 1.0);
  p.HP.assign(p.N + 1, 0);
  for (int t = 0; t + 1 < p.N; ++t)
    p.HP[t + 1] = p.HP[t] + per[t];
  p.HP[p.N] = p.HP[p.N - 1];
  p.nh = p.HP[p.N];
  p.HM.clear();
  for (int h = 0; h < p.nh; ++h)
  {
    int mk = 0;
    for (int e = 0; e < 2 * p.D; ++e)
      mk |= (u(rng) < density) << e;
    p.HM.push_back(mk);
  }
  if (p.HM.empty())
    p.HM.push_back(0);
}

// A pair that differs in exactly one row index: entry ki + delta holds row r in oa and r + 1 in ob (a mask bit
// moved to the next row of the same waypoint or step pair: the column keeps its count, so every pointer and nnz
// stay), with nnz % 8 = kir.  hinge_row: the entry is a hinge row, else an abs row.  first: it is its column's
// first entry (the walk meets the prefix's end at its first group).
bool row_boundary_pair(Pattern a, int delta, int kir, bool hinge_row, bool first, Pattern& oa, Pattern& ob)
{
  std::vector<int64_t> cp, ci;
  build_csc(a, cp, ci);
  const long long nnz = static_cast<long long>(ci.size());
  struct Cand
  {
    int row, next, bit, t_col;
    long long E;
  } best{-1, -1, 0, 0, 0};
  long long best_d = -1;
  auto offer = [&](int row, int next, int bit, int col, int64_t rowval) {
    const long long E = entry_of(cp, ci, col, rowval);
    if (E < 1 || (first && E != cp[col]))
      return;
    long long d = 8 * (E - delta) + kir - nnz;
    d = d < 0 ? -d : d;
    if (best_d < 0 || d < best_d)
      best_d = d, best = Cand{row, next, bit, col / a.D, E};
  };
  if (!hinge_row)
  {
    for (int t = 0; t + 1 < a.N; ++t)
      for (int q = a.step_ptr[t]; q + 1 < a.step_ptr[t + 1]; ++q)
        for (int j = 0; j < a.D; ++j)
          if (((a.mask[a.step_rows[q]] >> j) & 1) && !((a.mask[a.step_rows[q + 1]] >> j) & 1))
            offer(a.step_rows[q], a.step_rows[q + 1], j, t * a.D + j, a.n_fixed_rows + a.step_rows[q]);
  }
  else
  {
    for (int t = 0; t + 2 < a.N; ++t)
      for (int h = a.HP[t]; h + 1 < a.HP[t + 1]; ++h)
        for (int e = 0; e < 2 * a.D; ++e)
          if (((a.HM[h] >> e) & 1) && !((a.HM[h + 1] >> e) & 1))
            offer(h, h + 1, e, (t + e / a.D) * a.D + e % a.D, a.n_rows() + h);
  }
  if (best_d < 0 || !tune_nnz(a, best.t_col, 8 * (best.E - delta) + kir))
    return false;
  oa = ob = a;
  std::vector<int>& m = hinge_row ? ob.HM : ob.mask;
  m[best.row] &= ~(1 << best.bit);
  m[best.next] |= 1 << best.bit;
  const FpPrefix P = literal_prefix(oa.n(), nnz_of(oa));
  return P.ki + delta == best.E && P.kir == kir && nnz_of(ob) == nnz_of(oa);
}

// A pair that differs in exactly one column pointer, p[kp + delta] (a mask bit moved from column kp + delta - 1
// to column kp + delta in the same row), with (n + 1) % 8 = kpr and every row index inside the row prefix unchanged
bool ptr_boundary_pair(Pattern a, int delta, int kpr, std::mt19937_64& rng, Pattern& oa, Pattern& ob)
{
  if (!a.hinge || a.nh == 0 || a.N < 3)
    return false;
  while ((a.n() + 1) % 8 != kpr)  // one more hinge row in the last step pair
  {
    a.HM.push_back(static_cast<int>(rng() % (1u << (2 * a.D))));
    a.nh++;
    a.HP[a.N - 1]++;
    a.HP[a.N]++;
  }
  const int c = (a.n() + 1) / 8 + delta;
  if (c < 1 || c >= a.nx())
    return false;
  std::vector<int64_t> cp, ci;
  build_csc(a, cp, ci);
  if (cp[c - 1] <= static_cast<int64_t>(ci.size() / 8) + 1)
    return false;  // the change would reach into the row prefix
  const int t = c / a.D, j = c % a.D;
  oa = ob = a;
  if (j >= 1)
  {
    for (int q = a.step_ptr[t]; q < a.step_ptr[t + 1]; ++q)
      if (move_bit(ob.mask[a.step_rows[q]], j - 1, j))
        return true;
    if (t + 1 < a.N)
      for (int h = a.HP[t]; h < a.HP[t + 1]; ++h)
        if (move_bit(ob.HM[h], j - 1, j))
          return true;
    if (t > 0)
      for (int h = a.HP[t - 1]; h < a.HP[t]; ++h)
        if (move_bit(ob.HM[h], a.D + j - 1, a.D + j))
          return true;
    return false;
  }
  for (int h = a.HP[t - 1]; h < a.HP[t]; ++h)  // column (t - 1, D - 1) to column (t, 0): a row of pair t - 1
    if (move_bit(ob.HM[h], a.D - 1, a.D))
      return true;
  return false;
}

// p[kp] changed by -moved with (n + 1) % 8 = 1 (only its lowest byte is compared): `moved` hinge rows of the
// step pair of column kp move their bit from column kp - 1 to column kp.  Every other pointer, nnz and the row
// prefix stay.  moved = 256 changes byte 1 alone.
bool ptr_bytes_pair(std::mt19937_64& rng, int moved, Pattern& oa, Pattern& ob)
{
  const int D = 7, N = 30;
  Pattern a = make_pattern(rng, D, N, 6, 0, 1, 0.5);
  for (int H = 600; H < 700; ++H)
  {
    const int n = a.nc_base() + H;
    const int c = (n + 1) / 8, t = c / D, j = c % D;
    if (n % 8 != 0 || j < 1 || c >= a.nx() || t > N - 2)
      continue;
    std::vector<int> per(N - 1, 10);
    per[t] = H - 10 * (N - 2);
    set_hinge(a, per, rng, 0.5);
    for (int k = 0; k < 256; ++k)
      a.HM[a.HP[t] + k] = (a.HM[a.HP[t] + k] | (1 << (j - 1))) & ~(1 << j);
    std::vector<int64_t> cp, ci;
    build_csc(a, cp, ci);
    if (cp[c - 1] <= static_cast<int64_t>(ci.size() / 8) + 1)
      return false;
    oa = ob = a;
    for (int k = 0; k < moved; ++k)
      if (!move_bit(ob.HM[a.HP[t] + k], j - 1, j))
        return false;
    return (oa.n() + 1) % 8 == 1 && (oa.n() + 1) / 8 == c;
  }
  return false;
}

// Entry ki holds hinge row h0 in oa and h0 + 256 in ob (the rows between have no entry in that column), with
// nnz % 8 = kir: the two row indices differ in byte 1 alone
bool row_bytes_pair(std::mt19937_64& rng, int kir, Pattern& oa, Pattern& ob)
{
  const int D = 7, N = 30;
  for (int T = 2; T + 3 < N; ++T)
  {
    Pattern a = make_pattern(rng, D, N, 1, 0, 1, 0.5);
    std::vector<int> per(N - 1, 6);
    per[T] = 300;
    set_hinge(a, per, rng, 0.15);
    const int h0 = a.HP[T] + 5;
    for (int k = 0; k <= 256; ++k)
      a.HM[h0 + k] &= ~1;  // column (T, 0)
    a.HM[h0] |= 1;
    std::vector<int64_t> cp, ci;
    build_csc(a, cp, ci);
    const long long E = entry_of(cp, ci, T * D, a.n_rows() + h0);
    if (E < 0 || !tune_nnz(a, T + 1, 8 * E + kir))
      continue;
    oa = ob = a;
    ob.HM[h0] &= ~1;
    ob.HM[h0 + 256] |= 1;
    const FpPrefix P = literal_prefix(oa.n(), nnz_of(oa));
    return P.ki == E && P.kir == kir && ((oa.n_rows() + h0) & 255) == ((oa.n_rows() + h0 + 256) & 255);
  }
  return false;
}

struct Shape
{
  const char* name;
  int D, N, rows_per_step, nh, hinge;
};
}  // namespace

int main()
{
  std::mt19937_64 rng(20261020);
  const Shape shapes[] = {
      {"C-like 30 waypoints", 7, 30, 6, 120, 1},   {"30 waypoints, many hinge rows", 7, 30, 6, 758, 1},
      {"30 waypoints, no hinge row", 7, 30, 6, 0, 1}, {"B-like (no hinge)", 7, 30, 6, 0, 0},
      {"3 waypoints", 7, 3, 6, 40, 1},             {"3 waypoints, 160 hinge rows", 7, 3, 2, 160, 1},
      {"3 waypoints, 450 hinge rows", 7, 3, 1, 450, 1}, {"3 waypoints, no abs row", 7, 3, 0, 30, 1},
      {"D = 8", 8, 10, 6, 60, 1},                  {"50 waypoints (two column chunks)", 7, 50, 6, 200, 1},
      {"14 dof", 14, 20, 6, 90, 1},
  };
  int bad = 0;
  int ends_x = 0, ends_aux = 0, ends_hinge = 0, kpr0 = 0, kir0 = 0;
  Tally same, inside, outside, hmove, hbit, fresh, sizes;
  for (const Shape& s : shapes)
  {
    for (int rep = 0; rep < 24; ++rep)
    {
      // rep >= 16: hinge counts stepped so that (n + 1) % 8 == 0 occurs; masks nudged until nnz % 8 == 0
      const int nh = (s.nh > 0 && rep >= 16) ? s.nh + (rep - 16) : s.nh;
      Pattern a = make_pattern(rng, s.D, s.N, s.rows_per_step, nh, s.hinge, 0.3 + 0.05 * (rep % 8));
      if (rep % 3 == 2 && a.n_abs > 0)
        for (int k = 0; k < 8 && fingerprint_wg(a).nnz % 8 != 0; ++k)
          a.mask[rng() % a.n_abs] ^= 1 << (rng() % a.D);
      const FpPrefix P = literal_prefix(a.n(), static_cast<long long>(nnz_of(a)));
      ends_x += P.kp < a.nx();
      ends_aux += P.kp >= a.nx() && P.kp < a.nc_base();
      ends_hinge += P.kp >= a.nc_base();
      kpr0 += P.kpr == 0;
      kir0 += P.kir == 0;
      const std::string tag = std::string(s.name) + " #" + std::to_string(rep);
      check_pair(tag + " identical", a, a, same);
      Pattern b = a;
      if (a.n_abs > 0 && move_abs_bit(b, 0, rng))
        check_pair(tag + " abs bit moved at the first waypoint", a, b, inside);
      b = a;
      if (a.n_abs > 0 && move_abs_bit(b, a.N - 1, rng))
        check_pair(tag + " abs bit moved at the last waypoint", a, b, outside);
      if (a.nh > 1)
      {
        b = a;
        if (move_hinge_bit(b, 0, rng))
          check_pair(tag + " bit of the first hinge row moved", a, b, hbit);
        b = a;
        if (move_hinge_bit(b, a.nh - 1, rng))
          check_pair(tag + " bit of the last hinge row moved", a, b, outside);
        // the last row of a step pair becomes the first of the next pair: early and late pairs
        for (int t : {0, a.N / 2, a.N - 3})
          if (t >= 0 && t + 2 < a.N && a.HP[t + 1] > a.HP[t])
          {
            b = a;
            b.HP[t + 1]--;
            check_pair(tag + " hinge row moved from pair " + std::to_string(t), a, b, hmove);
          }
      }
      Pattern c2 = make_pattern(rng, s.D, s.N, s.rows_per_step, nh, s.hinge, 0.3 + 0.05 * (rep % 8));
      check_pair(tag + " another pattern of the same shape", a, c2, fresh);
      Pattern c3 = make_pattern(rng, s.D, s.N, s.rows_per_step, nh + 1 + static_cast<int>(rng() % 3), s.hinge, 0.5);
      check_pair(tag + " another number of hinge rows", a, c3, sizes);
    }
  }
  // one element changed at a chosen distance from a prefix's end
  Tally row_in, row_at, row_at_free, row_out, ptr_in, ptr_at, ptr_at_free, ptr_out, bytes_high, bytes_low;
  int row_first = 0, row_hinge = 0, row_abs = 0;
  const Shape edge_shapes[] = {{"C-like", 7, 30, 6, 120, 1}, {"many hinge rows", 7, 30, 6, 758, 1},
                               {"D = 8", 8, 10, 6, 60, 1},   {"50 waypoints", 7, 50, 6, 200, 1}};
  for (const Shape& s : edge_shapes)
    for (int rep = 0; rep < 4; ++rep)
    {
      const Pattern base = make_pattern(rng, s.D, s.N, s.rows_per_step, s.nh, s.hinge, 0.35 + 0.1 * rep);
      Pattern a, b;
      for (int rest : {0, 1, 3, 7})
        for (int delta : {-1, 0, 1})
        {
          for (int kind = 0; kind < 4; ++kind)  // abs / hinge row, anywhere / first of its column
            if (row_boundary_pair(base, delta, rest, kind & 1, kind & 2, a, b))
            {
              const std::string tag = std::string(s.name) + " row entry ki" + (delta < 0 ? " - 1" : delta ? " + 1" : "") +
                                      ", kir " + std::to_string(rest) + ", kind " + std::to_string(kind);
              const bool eq = delta > 0 || (delta == 0 && rest == 0);
              check_expect(tag, a, b, delta < 0 ? row_in : delta > 0 ? row_out : rest ? row_at : row_at_free, eq);
              row_first += (kind & 2) && delta == 0 && rest;
              row_hinge += kind & 1;
              row_abs += !(kind & 1);
            }
          if (ptr_boundary_pair(base, delta, rest, rng, a, b))
          {
            const std::string tag = std::string(s.name) + " pointer kp" + (delta < 0 ? " - 1" : delta ? " + 1" : "") +
                                    ", kpr " + std::to_string(rest);
            const bool eq = delta > 0 || (delta == 0 && rest == 0);
            check_expect(tag, a, b, delta < 0 ? ptr_in : delta > 0 ? ptr_out : rest ? ptr_at : ptr_at_free, eq);
          }
        }
    }
  {
    Pattern a, b;
    for (int rep = 0; rep < 3; ++rep)
    {
      if (ptr_bytes_pair(rng, 256, a, b))
        check_expect("p[kp] changed by 256 with kpr = 1", a, b, bytes_high, true);
      if (ptr_bytes_pair(rng, 1, a, b))
        check_expect("p[kp] changed by 1 with kpr = 1", a, b, bytes_low, false);
      if (ptr_bytes_pair(rng, 255, a, b))
        check_expect("p[kp] changed by 255 with kpr = 1", a, b, bytes_low, false);
      if (row_bytes_pair(rng, 1, a, b))
        check_expect("i[ki] changed by 256 with kir = 1", a, b, bytes_high, true);
      if (row_bytes_pair(rng, 2, a, b))
        check_expect("i[ki] changed by 256 with kir = 2", a, b, bytes_low, false);
    }
  }
  for (const Tally* t : {&same, &inside, &outside, &hmove, &hbit, &fresh, &sizes, &row_in, &row_at, &row_at_free, &row_out,
                         &ptr_in, &ptr_at, &ptr_at_free, &ptr_out, &bytes_high, &bytes_low})
    bad += t->bad;
  auto need = [&](bool cond, const char* what) {
    if (!cond)
    {
      std::printf("FAIL the cases hold no %s\n", what);
      ++bad;
    }
  };
  need(same.equal == same.pairs && same.pairs > 0, "identical pair that compares equal every time");
  need(inside.pairs > inside.equal && inside.pairs > 0, "change inside the prefix that compares unequal");
  need(outside.equal > 0, "change outside the prefix that still compares equal");
  need(outside.pairs > outside.equal, "change of a late row that compares unequal (short problems)");
  need(hmove.pairs > hmove.equal && hmove.equal > 0, "hinge row moved between pairs with both outcomes");
  need(hbit.pairs > hbit.equal, "hinge bit change inside the prefix");
  need(ends_x > 0 && ends_aux > 0 && ends_hinge > 0, "pointer prefix ending in each of the three column groups");
  need(kpr0 > 0, "shape with (n + 1) % 8 == 0");
  need(kir0 > 0, "shape with nnz % 8 == 0");
  need(row_in.pairs >= 8 && row_at.pairs >= 8 && row_at_free.pairs >= 4 && row_out.pairs >= 8,
       "pairs that differ in row entry ki - 1, ki (kir > 0 and kir = 0) and ki + 1 alone");
  need(row_first > 0 && row_hinge > 0 && row_abs > 0, "row-entry pairs on abs rows, hinge rows and a column's first entry");
  need(ptr_in.pairs >= 4 && ptr_at.pairs >= 4 && ptr_at_free.pairs >= 2 && ptr_out.pairs >= 4,
       "pairs that differ in pointer kp - 1, kp (kpr > 0 and kpr = 0) and kp + 1 alone");
  need(bytes_high.pairs >= 4 && bytes_high.equal == bytes_high.pairs, "changes above the compared bytes of a partial element");
  need(bytes_low.pairs >= 6 && bytes_low.equal == 0, "changes in the compared bytes of a partial element");
  std::printf("edge pairs (equal/pairs): row ki-1 %d/%d, ki masked %d/%d, ki with kir = 0 %d/%d, ki+1 %d/%d; pointer kp-1 "
              "%d/%d, kp masked %d/%d, kp with kpr = 0 %d/%d, kp+1 %d/%d; high bytes %d/%d, low bytes %d/%d\n",
              row_in.equal, row_in.pairs, row_at.equal, row_at.pairs, row_at_free.equal, row_at_free.pairs, row_out.equal,
              row_out.pairs, ptr_in.equal, ptr_in.pairs, ptr_at.equal, ptr_at.pairs, ptr_at_free.equal, ptr_at_free.pairs,
              ptr_out.equal, ptr_out.pairs, bytes_high.equal, bytes_high.pairs, bytes_low.equal, bytes_low.pairs);
  std::printf("%s identical %d/%d equal; inside %d/%d; outside %d/%d; hinge row moved %d/%d; hinge bit %d/%d; "
              "fresh %d/%d; sizes %d/%d; prefix ends x/aux/hinge %d/%d/%d; kpr = 0: %d, kir = 0: %d\n",
              bad ? "FAILED" : "ok", same.equal, same.pairs, inside.equal, inside.pairs, outside.equal, outside.pairs,
              hmove.equal, hmove.pairs, hbit.equal, hbit.pairs, fresh.equal, fresh.pairs, sizes.equal, sizes.pairs,
              ends_x, ends_aux, ends_hinge, kpr0, kir0);
  return bad ? 1 : 0;
}
