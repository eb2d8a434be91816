// fmx_mstats.h -- batched backward matching statistics and super-maximal exact-match seeds on the 32-bit engine
// (fmx_match_stats_batch*; included by fmx_query.hip).
//
// An ADDITION with no counterpart in the crate: fmx_suffix_match_batch (fmx_suffix.h) asked at EVERY end position of
// every pattern.  The work item is a SLOT, one per pattern symbol: slot t = off[k] - off[0] + i - 1 is end position i
// (1 <= i <= m) of pattern k, the prefix P[0 .. i).  For every slot:
//     (s, e) = (0, len); L = 0
//     for c in P[0 .. i) reversed:
//         if L == max_len: break                              # (a cap of 0 is none)
//         if c > max_character: break                         # ends the match, NOT an error
//         s' = lf_map2(c, s); e' = lf_map2(c, e)
//         if e' < s' or e' - s' < min_count: break
//         s = s'; e = e'; L += 1
//     out_len[t] = L; (out_s[t], out_e[t]) = L ? (s, e) : (0, 0)
// The shortcuts are those of fmx_suffix.h, for the same reason (interval sizes never grow along the loop): a k-mer table
// entry of >= min_count rows is the state after k steps, a pair probe that wide the state after two more.
//
// Three passes on one stream, nothing allocated:
//   1. out_len is set to all-ones, and fmx_ms_owner_kernel (a group per pattern, lanes striding over its symbols)
//      checks the offsets as the count kernels do and writes k into out_len[t] for the slots of valid patterns, below
//      `total` only.  A group of the main kernel so learns its pattern from one read instead of a binary search of
//      `off` per slot.
//   2. the main kernel (one per rung of the dispatch ladder, fmx_route in fmx_query.hip, that has a use here; 8-lane
//      groups striding over the SLOTS, so the groups of a wave take adjacent end positions of one pattern and share
//      its bytes and first record lines in cache) reads k = out_len[t], then off[k], and overwrites the slot with L.  An id that is no pattern's, or a slot
//      outside its pattern, is an unowned slot: zeros.  The kernel checks this itself and trusts nothing the owner
//      pass wrote.  With the seed filter on, lane 0 also sets FMX_MS_LAST in the word of a pattern's last slot.
//   3. fmx_ms_seed_kernel (elementwise; only with min_seed_len > 0 and out_s or out_e given) zeroes (s, e) of every
//      slot that is no seed and clears FMX_MS_LAST.  It reads out_len[t + 1] under that mask, so a neighbour clearing
//      its own bit meanwhile changes nothing it sees.
// `mc` is min_count clamped to 1 .. 2^32 - 1 and `cap` is max_len with 0 and everything above 2^32 - 1 turned into
// 2^32 - 1 by the launcher (a pattern has at most 2^32 - 1 symbols).
#pragma once

#define FMX_MS_LAST 0x8000000000000000ull   // out_len[t] between the main and the seed kernel: t is its pattern's last slot

// the offsets of every pattern checked once (FMX_ERR_ARG as in the count kernels); the owner id of every slot of a
// valid pattern, never at or above `total`
__global__ __launch_bounds__(FMX_BLOCK) void fmx_ms_owner_kernel(
    uint32_t *status, const uint64_t *__restrict__ off, uint64_t npat, uint64_t total, uint64_t *__restrict__ owner) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  const uint64_t ptot = off[npat], pmin = off[0];
  if (gid == 0 && g == 0 && (ptot < pmin || ptot - pmin != total)) atomicOr(status, 1u << FMX_ERR_ARG);
  for (uint64_t k = gid; k < npat; k += ngroups) {
    const uint64_t pbeg = off[k], pend = off[k + 1];
    if (FMX_SPAN_BAD32(pbeg, pend, pmin, ptot)) {
      if (g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
      continue;
    }
    const uint64_t t0 = pbeg - pmin, m = pend - pbeg;
    for (uint64_t i = g; i < m && t0 + i < total; i += FMX_GROUP) owner[t0 + i] = k;
  }
}

// slot t with the owner id k: its pattern's first symbol, its end position i and whether i == m.  false = unowned (an
// id that is no pattern's, offsets the count kernels refuse, a slot outside the pattern): nothing may be read for it.
__device__ __forceinline__ bool fmx_ms_slot(const uint64_t *__restrict__ off, uint64_t npat, uint64_t pmin,
                                            uint64_t ptot, uint64_t t, uint64_t k, uint64_t &pbeg, uint32_t &i,
                                            bool &last) {
  if (k >= npat) return false;
  pbeg = off[k];
  const uint64_t pend = off[k + 1];
  if (FMX_SPAN_BAD32(pbeg, pend, pmin, ptot)) return false;
  const uint64_t r = t + pmin - pbeg;                    // i - 1 (wraps to a huge value for a slot before the pattern)
  if (t + pmin < pbeg || r >= pend - pbeg) return false;
  i = (uint32_t)r + 1u;
  last = r + 1u == pend - pbeg;
  return true;
}

// group per slot, every kind and level count (the shape of fmx_sfx_kernel).  The run-length instantiations of the twin
// sit at 60-62 of the 64 registers that 8 waves per SIMD allow; with the slot state on top they would spill, so they
// are asked for 6 waves per SIMD here (they take 7).
template <int KIND, int NL, bool KM, int SM>
__global__ __launch_bounds__(FMX_BLOCK, KIND == FMX_KIND_RLFM ? 6 : 8) void fmx_ms_kernel(
    FmxDev ix, const void *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat, uint64_t total,
    uint32_t mc, uint32_t cap, uint64_t lastbit, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;

  uint64_t t = gid;          // current slot
  bool active = t < total;
  bool fresh = true;         // slot state not loaded yet
  uint64_t pbeg = 0;         // first symbol of the slot's pattern
  uint64_t lastw = 0;        // FMX_MS_LAST for a pattern's last slot when the seed filter follows
  uint32_t j = 0;            // symbols still to consume (from the back of the prefix)
  uint32_t s = 0, e = 0, len = 0;
  uint32_t c = 0;            // symbol of the coming step (loaded one step ahead)

  const uint64_t ptot = off[npat], pmin = off[0];
  uint64_t nk = active ? out_len[t] : 0;   // the owner id of the group's NEXT slot travels under the current slot's steps
  while (active) {
    if (fresh) {
      const uint64_t k = nk;
      if (t + ngroups < total) nk = out_len[t + ngroups];
      uint32_t i = 0;
      bool last = false;
      s = 0; e = ix.n; len = 0; j = 0; lastw = 0;
      if (fmx_ms_slot(off, npat, pmin, ptot, t, k, pbeg, i, last)) {
        lastw = last ? lastbit : 0ull;
        if (ix.n >= mc) j = i;                             // (a whole index below min_count: no step can pass)
        if (KM && j >= ix.kmer_k && cap >= ix.kmer_k) {    // all kmer_k symbols at once when the entry is wide enough
          uint32_t code;
          if (fmx_kmer_code((const uint8_t *)pat, pbeg + j, ix.kmer_k, ix.kmer_bits, ix.max_character, g, code)) {
            FMX_TOUCH_G0N(g, &ix.kmer[code]);
            const uint2 se = ix.kmer[code];
            if (se.y - se.x >= mc) { s = se.x; e = se.y; j -= ix.kmer_k; len = ix.kmer_k; }
          }
        }
        c = j ? fmx_load_sym(pat, ix.sym_bytes, pbeg + j - 1) : 0u;
      }
      fresh = false;
    }
    bool done = j == 0 || len >= cap || c > ix.max_character;   // an absent symbol ends the match
    if (!done) {
      // the next symbol rides along with this step's record loads
      const uint32_t cn = j > 1 ? fmx_load_sym(pat, ix.sym_bytes, pbeg + j - 2) : 0u;
      uint32_t ns = s, ne = e;
      fmx_lf_map2_pair<KIND, NL, SM>(ix, c, ns, ne, g);
      // (ne < ns: lf_map2(0, .) of a multi-pieces index is not monotone, multi_pieces.rs:147-153 -- below every min_count)
      if (ne < ns || ne - ns < mc) {
        done = true;                                     // keep the previous (s, e, len)
      } else {
        s = ns; e = ne; len++;
        c = cn;
        j--;
        done = j == 0;
      }
    }
    if (done) {
      if (g == 0) {
        if (out_s) out_s[t] = len ? s : 0u;
        if (out_e) out_e[t] = len ? e : 0u;
        out_len[t] = (uint64_t)len | lastw;
      }
      t += ngroups;
      active = t < total;
      fresh = true;
    }
  }
}

// the index of an EMPTY text: nothing matches, every slot is L = 0, (0, 0) (the offsets were checked by the owner pass)
__global__ __launch_bounds__(FMX_BLOCK) void fmx_ms_empty_kernel(
    uint64_t total, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_len) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    if (out_s) out_s[t] = 0;
    if (out_e) out_e[t] = 0;
    out_len[t] = 0;
  }
}

// single 3-bit level (DNA): one 128-byte line per interval end and step (the shape of fmx_sfx_f3_kernel)
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_ms_f3_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character,
    const uint2 *__restrict__ kmer, uint32_t kmer_k, uint32_t kmer_bits,
    const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat, uint64_t total,
    uint32_t mc, uint32_t cap, uint64_t lastbit, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  [[maybe_unused]] const uint32_t nrec = n / 256u + 1u;

  uint64_t t = gid, pbeg = 0, lastw = 0;
  bool active = t < total, fresh = true;
  uint32_t j = 0, s = 0, e = 0, c = 0, len = 0;
  const uint64_t ptot = off[npat], pmin = off[0];
  uint64_t nk = active ? out_len[t] : 0;   // the owner id of the group's NEXT slot travels under the current slot's steps
  while (active) {
    if (fresh) {
      const uint64_t k = nk;
      if (t + ngroups < total) nk = out_len[t + ngroups];
      uint32_t i = 0;
      bool last = false;
      s = 0; e = n; len = 0; j = 0; lastw = 0;
      if (fmx_ms_slot(off, npat, pmin, ptot, t, k, pbeg, i, last)) {
        lastw = last ? lastbit : 0ull;
        if (n >= mc) j = i;                                // (a whole index below min_count: no step can pass)
        if (KM && j >= kmer_k && cap >= kmer_k) {          // all kmer_k symbols at once when the entry is wide enough
          uint32_t code;
          if (fmx_kmer_code(pat, pbeg + j, kmer_k, kmer_bits, max_character, g, code)) {
            FMX_TOUCH_G0N(g, &kmer[code]);
            const uint2 se = kmer[code];
            if (se.y - se.x >= mc) { s = se.x; e = se.y; j -= kmer_k; len = kmer_k; }
          }
        }
        c = j ? pat[pbeg + j - 1] : 0u;                    // last symbol of the prefix first
      }
      fresh = false;
    }
    bool done = j == 0 || len >= cap || c > max_character; // an absent symbol ends the match
    if (!done) {
      const uint32_t rs = s >> 8, re = e >> 8;
      FMX_CHECK(rs < nrec && re < nrec);
      FMX_TOUCH_G0(g, &rec[(size_t)rs * 8u]);
      if (re != rs) FMX_TOUCH_G0(g, &rec[(size_t)re * 8u]);
      const uint4 a = rec[(size_t)rs * 8u + g];
      const uint4 b = rec[(size_t)re * 8u + g];
      const uint32_t cn = j > 1 ? pat[pbeg + j - 2] : 0u;    // rides along with the record loads
      const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(a, s & 255u, c, g));
      const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(b, e & 255u, c, g));
      if (ne - ns < mc) {
        done = true;                                     // keep the previous (s, e, len)
      } else {
        s = ns; e = ne; len++;
        c = cn;
        j--;
        done = j == 0;
      }
    }
    if (done) {
      if (g == 0) {
        if (out_s) out_s[t] = len ? s : 0u;
        if (out_e) out_e[t] = len ? e : 0u;
        out_len[t] = (uint64_t)len | lastw;
      }
      t += ngroups;
      active = t < total;
      fresh = true;
    }
  }
}

// the opt-in pair index (the shape of fmx_sfx_pair_kernel): while two symbols remain, both in 1..4, and the cap leaves
// room for two, one probe of the 2-gram records per interval end advances two symbols when its result keeps
// >= min_count rows.  Otherwise the single step for the last symbol on the 1-gram records: >= min_count rows -> taken,
// and after a failed pair probe the match ends there, the second symbol being known to fail; else nothing is taken.
// With one symbol of budget left no pair probe is made, so a pair step never overshoots the cap.
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_ms_pair_kernel(
    const uint4 *__restrict__ rec1, const uint4 *__restrict__ rec2, uint32_t n,
    uint32_t max_character, uint32_t row0, uint32_t row1,
    const uint2 *__restrict__ kmer, uint32_t kmer_k, uint32_t kmer_bits,
    const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat, uint64_t total,
    uint32_t mc, uint32_t cap, uint64_t lastbit, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;

  uint64_t t = gid, pbeg = 0, lastw = 0;
  bool active = t < total, fresh = true;
  uint32_t j = 0, s = 0, e = 0, len = 0;
  uint32_t c2 = 0, c1 = 0;   // c2 = last unread symbol, c1 = the one before it
  const uint64_t ptot = off[npat], pmin = off[0];
  uint64_t nk = active ? out_len[t] : 0;   // the owner id of the group's NEXT slot travels under the current slot's steps
  while (active) {
    if (fresh) {
      const uint64_t k = nk;
      if (t + ngroups < total) nk = out_len[t + ngroups];
      uint32_t i = 0;
      bool last = false;
      s = 0; e = n; len = 0; j = 0; lastw = 0;
      if (fmx_ms_slot(off, npat, pmin, ptot, t, k, pbeg, i, last)) {
        lastw = last ? lastbit : 0ull;
        if (n >= mc) j = i;                                // (a whole index below min_count: no step can pass)
        if (KM && j >= kmer_k && cap >= kmer_k) {          // all kmer_k symbols at once when the entry is wide enough
          uint32_t code;
          if (fmx_kmer_code(pat, pbeg + j, kmer_k, kmer_bits, max_character, g, code)) {
            FMX_TOUCH_G0N(g, &kmer[code]);
            const uint2 se = kmer[code];
            if (se.y - se.x >= mc) { s = se.x; e = se.y; j -= kmer_k; len = kmer_k; }
          }
        }
        c2 = j ? pat[pbeg + j - 1] : 0u;
        c1 = j > 1 ? pat[pbeg + j - 2] : 0u;
      }
      fresh = false;
    }
    bool done = j == 0 || len >= cap || c2 > max_character;  // an absent symbol ends the match
    if (!done) {
      const bool pair = j >= 2 && cap - len >= 2u && (c2 - 1u) < 4u && (c1 - 1u) < 4u && c1 <= max_character;
      // the two symbols after these ride along with the record loads
      const uint32_t n1 = j > 2 ? pat[pbeg + j - 3] : 0u;
      const uint32_t n2 = j > 3 ? pat[pbeg + j - 4] : 0u;
      uint32_t used = 0;
      if (pair) {
        const uint32_t code = (c1 - 1u) * 4u + (c2 - 1u);
        FMX_CHECK((s >> 7) < n / 128u + 1u && (e >> 7) < n / 128u + 1u);
        FMX_TOUCH_G0(g, &rec2[(size_t)(s >> 7) * 8u]);
        if ((e >> 7) != (s >> 7)) FMX_TOUCH_G0(g, &rec2[(size_t)(e >> 7) * 8u]);
        const uint4 a = rec2[(size_t)(s >> 7) * 8u + g];
        const uint4 b = rec2[(size_t)(e >> 7) * 8u + g];
        uint32_t ns = fmx_group_sum(fmx_piece_rank<4>(a, s & 127u, code, g));
        uint32_t ne = fmx_group_sum(fmx_piece_rank<4>(b, e & 127u, code, g));
        if (code == 0u) {  // the two rows without a 2-gram are stored as code 0
          ns -= (uint32_t)(s > row0) + (uint32_t)(s > row1);
          ne -= (uint32_t)(e > row0) + (uint32_t)(e > row1);
        }
        if (ne - ns >= mc) { s = ns; e = ne; used = 2; }
      }
      if (used == 0) {       // one symbol on the 1-gram records
        FMX_CHECK((s >> 8) < n / 256u + 1u && (e >> 8) < n / 256u + 1u);
        FMX_TOUCH_G0(g, &rec1[(size_t)(s >> 8) * 8u]);
        if ((e >> 8) != (s >> 8)) FMX_TOUCH_G0(g, &rec1[(size_t)(e >> 8) * 8u]);
        const uint4 a1 = rec1[(size_t)(s >> 8) * 8u + g];
        const uint4 b1 = rec1[(size_t)(e >> 8) * 8u + g];
        const uint32_t s1 = fmx_group_sum(fmx_piece_rank<3>(a1, s & 255u, c2, g));
        const uint32_t e1 = fmx_group_sum(fmx_piece_rank<3>(b1, e & 255u, c2, g));
        if (e1 - s1 >= mc) { s = s1; e = e1; used = 1; }
        done = pair || used == 0;                        // after a failed pair probe the second symbol is known to fail
      }
      len += used;
      j -= used;
      if (used == 2) { c2 = n1; c1 = n2; } else { c2 = c1; c1 = n1; }
      done |= j == 0;
    }
    if (done) {
      if (g == 0) {
        if (out_s) out_s[t] = len ? s : 0u;
        if (out_e) out_e[t] = len ? e : 0u;
        out_len[t] = (uint64_t)len | lastw;
      }
      t += ngroups;
      active = t < total;
      fresh = true;
    }
  }
}

// the seed filter, a lane per slot: slot t keeps its (s, e) when L[t] >= min_seed_len and the match is not contained
// in the one ending a symbol later (t is its pattern's last slot, or L[t + 1] <= L[t]).  out_len is only touched to
// clear the slot's own FMX_MS_LAST, and the neighbour's word is read under that mask: it is final and raw afterwards.
__global__ __launch_bounds__(FMX_BLOCK) void fmx_ms_seed_kernel(
    uint64_t total, uint64_t min_seed_len, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *out_len) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const uint64_t w = out_len[t];
    const bool last = (w & FMX_MS_LAST) != 0;
    const uint64_t len = w & ~FMX_MS_LAST;
    const uint64_t nxt = (last || t + 1 >= total) ? 0ull : out_len[t + 1] & ~FMX_MS_LAST;
    if (!(len >= min_seed_len && nxt <= len)) {
      if (out_s) out_s[t] = 0;
      if (out_e) out_e[t] = 0;
    }
    if (last) out_len[t] = len;
  }
}

// ---- launch: the ladder of fmx_route() (fmx_query.hip) without the endpoint-per-lane shape -- a run-length index takes
// the group kernel with hints + record search, which is valid for every vector.  The caller has refused a wide handle
// and a NULL d_len; npat > 0. ----
int fmx_launch_match_stats(const fmx_index *idx, const void *d_pat, const uint64_t *d_off, uint64_t npat,
                           uint64_t total, uint64_t min_count, uint64_t max_len, uint64_t min_seed_len,
                           uint64_t *d_s, uint64_t *d_e, uint64_t *d_len, hipStream_t st) {
  if (min_count == 0) min_count = 1;
  const FmxDev dv = fmx_launch_dev(idx);
  const bool seeds = min_seed_len > 0 && (d_s || d_e);
  if (total) FMX_HIP(hipMemsetAsync(d_len, 0xFF, (size_t)total * 8, st));
  hipLaunchKernelGGL(fmx_ms_owner_kernel, dim3(fmx_grid_for_groups(npat)), dim3(FMX_BLOCK), 0, st, dv.status, d_off,
                     npat, total, d_len);
  FMX_HIP(hipGetLastError());
  if (total == 0) return FMX_OK;                     // (the owner pass has compared the offsets with it)
  if (idx->n == 0) {                                 // no record of any structure may be probed
    hipLaunchKernelGGL(fmx_ms_empty_kernel, dim3(fmx_grid_for_groups((total + 7) / 8)), dim3(FMX_BLOCK), 0, st, total,
                       d_s, d_e, d_len);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }
  const FmxRoute r = fmx_route(idx, dv, fmx_tune(), FMX_SHAPE_PAIR | FMX_SHAPE_F3 | FMX_SHAPE_GROUP | FMX_HAS_KMER);
  const uint32_t mc = min_count > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)min_count;
  const uint32_t cap = (max_len == 0 || max_len > 0xFFFFFFFFull) ? 0xFFFFFFFFu : (uint32_t)max_len;
  const uint64_t lastbit = seeds ? FMX_MS_LAST : 0ull;
  const dim3 grid(fmx_grid_for_groups(total)), block(FMX_BLOCK);
  const uint8_t *pat8 = (const uint8_t *)d_pat;
  if (r.shape == FMX_SHAPE_PAIR) {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_ms_pair_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.pair_rec, dv.n,
                         dv.max_character, dv.pair_row0, dv.pair_row1, dv.kmer, dv.kmer_k, dv.kmer_bits, pat8, d_off, npat,
                         total, mc, cap, lastbit, d_s, d_e, d_len);
    });
  } else if (r.shape == FMX_SHAPE_F3) {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_ms_f3_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.n, dv.max_character, dv.kmer,
                         dv.kmer_k, dv.kmer_bits, pat8, d_off, npat, total, mc, cap, lastbit, d_s, d_e, d_len);
    });
  } else {
    fmx_route_group(r, [&](auto kind, auto nl, auto sm, auto km) {
      hipLaunchKernelGGL((fmx_ms_kernel<kind(), nl(), km(), sm()>), grid, block, 0, st, dv, d_pat, d_off, npat, total, mc,
                         cap, lastbit, d_s, d_e, d_len);
    });
  }
  FMX_HIP(hipGetLastError());
  if (seeds) {
    hipLaunchKernelGGL(fmx_ms_seed_kernel, dim3(fmx_grid_for_groups((total + 7) / 8)), dim3(FMX_BLOCK), 0, st, total,
                       min_seed_len, d_s, d_e, d_len);
    FMX_HIP(hipGetLastError());
  }
  return FMX_OK;
}
