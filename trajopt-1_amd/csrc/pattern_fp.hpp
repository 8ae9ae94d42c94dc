// OSQPModel's sparsity fingerprint of the QP's constraint matrix A, as a sum
// over the compared elements (sqp_kernel.hip pattern_fingerprint_wg; host and
// device code, also compiled by host/tests/pattern_fp_check.cpp, which runs it
// "thread by thread" against a memcmp of the CSC arrays).
//
// OSQPModel (quirk Q2) counts A as unchanged when n, m and nnz are equal and
// the first n + 1 BYTES of its 64-bit column pointers and the first nnz BYTES
// of its 64-bit row indices are equal.  The compared elements are therefore
//   column pointer p[col] for col < kp, and the low kpr bytes of p[kp],
//   row index i[e] for e < ki, and the low kir bytes of i[ki],
// with kp = (n + 1) / 8, kpr = (n + 1) % 8, ki = nnz / 8, kir = nnz % 8.  The
// fingerprint is the wrapping 64-bit sum of fp_elem(tag, position, value) over
// them: the sum does not depend on the order, so every column can add its own
// elements once it knows its first entry number.
//
// A's CSC order: x columns waypoint-major, then two aux columns per abs row,
// then one column per hinge row; rows fixed < abs < hinge < identity block.
// x column (t, j): the fixed row of waypoint t, the waypoint's abs rows whose
// mask has bit j, the hinge rows of step pair t - 1 with bit D + j, those of
// pair t with bit j, the identity row.  Columns >= nx hold two entries each.
#pragma once

#if defined(__HIPCC__)
#define FP_HD __host__ __device__ __forceinline__
#define FP_UNROLL _Pragma("unroll")
#else
#define FP_HD inline
#define FP_UNROLL
#endif

namespace thip
{
struct FpDims
{
  int D, N, nx, nc_base, n_fixed_rows, n_rows, nh, hinge;
  FP_HD int n() const { return nc_base + nh; }
  FP_HD long long row_hinge0() const { return n_rows; }
  FP_HD long long row_ident0() const { return static_cast<long long>(n_rows) + nh; }
};

struct FpPrefix
{
  long long kp, kpr, ki, kir;
};

FP_HD FpPrefix fp_prefix(int n, long long nnz)
{
  FpPrefix P;
  P.kp = (n + 1) / 8;
  P.kpr = (n + 1) % 8;
  P.ki = nnz / 8;
  P.kir = nnz % 8;
  return P;
}

FP_HD unsigned long long fp_low(unsigned long long v, long long bytes)
{
  return bytes >= 8 ? v : (v & ((1ULL << (8 * bytes)) - 1ULL));
}

FP_HD unsigned long long fp_fin(unsigned long long z)
{
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// tag 0: column pointer, 1: row index
FP_HD unsigned long long fp_elem(int tag, long long pos, unsigned long long v)
{
  const unsigned long long k = fp_fin(0x9E3779B97F4A7C15ULL * (2ULL * static_cast<unsigned long long>(pos) + tag + 1ULL));
  return fp_fin(k + v);
}

// column pointer col's share of the fingerprint (0 past the compared prefix)
FP_HD unsigned long long fp_ptr_term(const FpPrefix& P, long long col, long long ptr)
{
  if (col < P.kp)
    return fp_elem(0, col, static_cast<unsigned long long>(ptr));
  if (col == P.kp && P.kpr)
    return fp_elem(0, col, fp_low(static_cast<unsigned long long>(ptr), P.kpr));
  return 0;
}

// entry e's (row index) share
FP_HD unsigned long long fp_row_term(const FpPrefix& P, long long e, long long row)
{
  if (e < P.ki)
    return fp_elem(1, e, static_cast<unsigned long long>(row));
  if (e == P.ki && P.kir)
    return fp_elem(1, e, fp_low(static_cast<unsigned long long>(row), P.kir));
  return 0;
}

FP_HD int fp_popc(int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(v);
#else
  return __builtin_popcount(static_cast<unsigned>(v));
#endif
}

// nnz from the sum of popc over the abs rows' masks and the hinge rows' masks
FP_HD long long fp_nnz(const FpDims& d, int n_abs, long long bits) { return static_cast<long long>(d.n_fixed_rows) + 2LL * n_abs + d.nh + d.n() + bits; }

// Rows q0 <= q < q1 of a list (row id idx[q], or q itself with INDIRECT
// false) that have bit `bit` of bits[row]: their number, and with HASH their
// share as entries e, e + 1, ... of row index row0 + row (e advances).  Eight
// rows at a time, every load of a group before its first use, from indices
// clamped into the list.
template <bool HASH, bool INDIRECT, class IP>
FP_HD int fp_walk(IP idx, IP bits, int q0, int q1, int bit, long long row0, const FpPrefix& P, long long& e,
                  unsigned long long& acc)
{
  int cnt = 0;
  for (int q = q0; q < q1; q += 8)
  {
    if (HASH && e > P.ki)
      break;  // every later entry lies past the compared prefix
    int r[8], mk[8];
    FP_UNROLL
    for (int k = 0; k < 8; ++k)
    {
      const int qq = (q + k < q1) ? q + k : q1 - 1;
      r[k] = INDIRECT ? idx[qq] : qq;
    }
    FP_UNROLL
    for (int k = 0; k < 8; ++k)
      mk[k] = bits[r[k]];
    FP_UNROLL
    for (int k = 0; k < 8; ++k)
    {
      const int on = (q + k < q1) ? ((mk[k] >> bit) & 1) : 0;
      if (HASH && on)
      {
        acc += fp_row_term(P, e, row0 + r[k]);
        ++e;
      }
      cnt += on;
    }
  }
  return cnt;
}

// x column col (< nx): its number of entries; with HASH also the share of its
// row indices, the first of which is entry e0 (skipped when e0 > ki).
template <bool HASH, class IP>
FP_HD int fp_x_column(const FpDims& d, IP fos, IP step_ptr, IP step_rows, IP mask, IP HP, IP HM, int col,
                      const FpPrefix& P, long long e0, unsigned long long& acc)
{
  if (HASH && e0 > P.ki)
    return 0;
  const int t = col / d.D, j = col % d.D;
  long long e = e0;
  int cnt = 0;
  const int f = fos[t];
  if (f >= 0)
  {
    if (HASH)
      acc += fp_row_term(P, e++, static_cast<long long>(f) * d.D + j);
    ++cnt;
  }
  cnt += fp_walk<HASH, true>(step_rows, mask, step_ptr[t], step_ptr[t + 1], j, d.n_fixed_rows, P, e, acc);
  if (d.hinge)
  {
    const int h0 = (t > 0) ? HP[t - 1] : 0, h1 = HP[t], h2 = (t < d.N - 1) ? HP[t + 1] : h1;
    if (t > 0)
      cnt += fp_walk<HASH, false>(HM, HM, h0, h1, d.D + j, d.row_hinge0(), P, e, acc);
    if (t < d.N - 1)
      cnt += fp_walk<HASH, false>(HM, HM, h1, h2, j, d.row_hinge0(), P, e, acc);
  }
  if (HASH)
    acc += fp_row_term(P, e, d.row_ident0() + col);
  return cnt + 1;
}

// Columns >= nx hold two entries each: the abs row (col - nx) / 2 for an aux
// column or the hinge row col - nc_base for a hinge column, then the identity
// row.  Every mask bit is an entry of an x column, so p[nx] = nnz - 2 (n - nx)
// and these columns' pointers and rows follow from (n, m, nnz) alone: between
// two set-ups whose n, m and nnz are equal (compared beside the hash) their
// terms are equal too and never change a decision.  They are summed all the
// same, so that the fingerprint covers exactly the compared elements and does
// not lean on what else is compared.  With p_nx the pointer of column nx:
FP_HD long long fp_tail_ptr(const FpDims& d, long long p_nx, int col) { return p_nx + 2LL * (col - d.nx); }
FP_HD long long fp_tail_row(const FpDims& d, int col)
{
  return col < d.nc_base ? static_cast<long long>(d.n_fixed_rows) + (col - d.nx) / 2 : d.row_hinge0() + (col - d.nc_base);
}
// the last column >= nx whose pointer or entries can lie inside a prefix
FP_HD int fp_tail_last(const FpDims& d, const FpPrefix& P, long long p_nx)
{
  long long last = P.kp;  // pointers: col <= kp (kp <= n)
  const long long by_e = d.nx + (P.ki - p_nx) / 2;  // entries: p[col] <= ki
  if (P.ki >= p_nx && by_e > last)
    last = by_e;
  return static_cast<int>(last < d.n() ? last : d.n());
}
// column col's (nx <= col <= n; col = n is the end pointer) share
FP_HD unsigned long long fp_tail_column(const FpDims& d, const FpPrefix& P, long long p_nx, int col)
{
  const long long p = fp_tail_ptr(d, p_nx, col);
  unsigned long long acc = fp_ptr_term(P, col, p);
  if (col < d.n() && p <= P.ki)
    acc += fp_row_term(P, p, fp_tail_row(d, col)) + fp_row_term(P, p + 1, d.row_ident0() + col);
  return acc;
}
}  // namespace thip
