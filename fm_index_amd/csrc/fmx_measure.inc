// fmx_measure.inc -- measurement builds only (-DFMX_MEASURE: make measure / make debug); never part of
// libfmx.so.  Included by fmx_query.hip right before its launchers.  Holds
//   * fmx_tune(): the dispatch choices of FmxTune read from FMX_VARIANT and the grid knobs, so that the
//     alternatives DESIGN.md section 4.1 quotes stay reproducible;
//   * the alternative kernels themselves and their launches (fmx_measure_count / fmx_measure_locate).
// FMX_VARIANT:
//   unset / 1  the shipped paths
//   0          the round-1 generic group-per-pattern / group-per-walk kernels (any kind, any number of levels)
//   2, 5       DNA count with 2 / 4 independent chains per group            (slower: 0.78 / 1.00 ms)
//   3, 4       DNA count skipping the 2nd load when both ends share a record (slower: 0.74 / 0.80 ms)
//   6          ignore the k-mer start table even when it was built
//   7          ignore the pair index even when it was built
//   8, 9       lane-per-pattern / wavefront-per-pattern DNA count kernels
//   11, 12, 14, 15  DNA locate with 1 / 2 / 4 / 8 walks per group
//   16, 17     (builder, fmx_build.hip) no stored positions / no select blocks for the RLFM bit vectors
//   20         endpoint-per-lane count on FM indexes;  21  one-walk-per-lane locate on the one-level index
//   22         DNA walk kernel of rounds 1-2 (state repeated in all 8 lanes);  23  hand-over at the end of the round
//   24, 25     distributed-state DNA count kernel with 4 / 2 patterns per group;  26  positions stored directly
//   27         text-order DNA walk through the phase pieces although the index has walk records
//   28         DNA walk records through the round-4 pair of launches instead of the one-launch kernel (FMX_ADJ_CLUSTERS:
//              runs of consecutive rows a 64-hit ticket may have and still be walked a lane per hit; 0 = never)
// (18 / 19, row- / text-order sampling, are build flags of the shipped library now: FMX_FLAG_ROW_ORDER /
// FMX_FLAG_TEXT_ORDER) and the grid knobs FMX_EP_BLOCKS, FMX_LOC_BLOCKS, FMX_LOC_THREADS, FMX_EP_LOC_BLOCKS,
// FMX_EP_LOC_THREADS, FMX_RL_EP_MIN, FMX_FM_EP_MIN (benchmarks/gpu/README.md).
#include <cstdlib>

static inline long fmx_env_long(const char *name, long dflt) {
  const char *v = getenv(name);
  return v ? atol(v) : dflt;
}
static inline FmxTune fmx_tune() {
  FmxTune t;
  const int v = (int)fmx_env_long("FMX_VARIANT", 1);
  t.generic = v == 0;
  t.use_kmer = v != 6;
  t.use_pair = v != 7;
  t.wc = v != 26;
  t.unified = v != 28;              // 28: the round-4 pair of launches (fmx_expand_kernel + f3t / lane kernel by batch average)
  t.adj_clusters = fmx_env_long("FMX_ADJ_CLUSTERS", t.adj_clusters);
  t.rl_lane_avg = v == 28 ? 64 : fmx_env_long("FMX_RL_LANE_AVG", t.rl_lane_avg);
  t.rl_unified = v == 28 ? false : fmx_env_long("FMX_RL_UNIFIED", 0) != 0;
  t.rl_rounds = fmx_env_long("FMX_RL_ROUNDS", 1) != 0;
  t.rl_rounds_blocks = fmx_env_long("FMX_RL_ROUNDS_BLOCKS", t.rl_rounds_blocks);
  t.walk_records = v != 27;         // 27: the round-3 text-order walk (phase probes) on an index that has walk records
  t.walks = v == 11 ? 1 : v == 12 ? 2 : v == 14 ? 4 : v == 15 ? 8 : 0;
  t.alt = (v == 2 || v == 3 || v == 4 || v == 5 || v == 8 || v == 9 || v == 15 || v == 20 || v == 21 || v == 22 ||
           v == 23 || v == 24 || v == 25 || v == 0) ? (v == 0 ? 100 : v) : 0;
  t.ep_blocks = fmx_env_long("FMX_EP_BLOCKS", t.ep_blocks);
  t.loc_blocks = fmx_env_long("FMX_LOC_BLOCKS", 0);
  t.loc_threads = fmx_env_long("FMX_LOC_THREADS", t.loc_threads);
  t.ep_loc_blocks = fmx_env_long("FMX_EP_LOC_BLOCKS", 0);
  t.ep_loc_threads = fmx_env_long("FMX_EP_LOC_THREADS", 0);
  t.rl_ep_min = fmx_env_long("FMX_RL_EP_MIN", t.rl_ep_min);
  t.fm_ep_min = fmx_env_long("FMX_FM_EP_MIN", t.fm_ep_min);
  return t;
}

// ---------------------------------------------------------------------------
// The same count with the PATTERN STATE DISTRIBUTED over the lanes of a group (the form the DNA walk
// kernel takes, fmx_locate_f3p_kernel): a group of 8 lanes still reads one 128-byte record per interval
// end, but it advances Q patterns at a time and lane q of each quad keeps pattern q -- its offsets, the
// symbols still to consume, (s, e) -- so fetching the next symbol, the early exit (wrapper.rs:111-113),
// the outputs and the start of the next pattern run once per round for all Q, lane-wise, and only the
// two record loads + the two rank decodes run per pattern (s, e, c broadcast inside the quad).
// No k-mer table here (that lookup is cooperative over the group): fmx_count_f3_kernel serves it.
// ---------------------------------------------------------------------------
template <int Q>
__device__ __forceinline__ uint32_t fmx_slot_bcast(uint32_t v, int q) {
  return Q == 1 ? v : fmx_quad_bcast(v, q);
}
template <int Q>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_count_f3d_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character, uint32_t *status,
    const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    const uint64_t *__restrict__ s0e0, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ steps_out) {
  static_assert(Q == 2 || Q == 4, "patterns per group");
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  [[maybe_unused]] const uint32_t nrec = n / 256u + 1u;
  const uint32_t slot = g & (uint32_t)(Q - 1);        // the pattern whose state this lane keeps (8 / Q replicas)
  const bool owner = g < (uint32_t)Q;                 // the replica that stores and counts
  constexpr unsigned long long SLOT0 = Q == 4 ? 0x1111111111111111ull : 0x5555555555555555ull;
  constexpr uint32_t NONE = 0xFFFFFFFFu;              // not a position (n < 2^32 - 16)
  const uint64_t ptot = npat ? off[npat] : 0;         // symbols the caller declares behind `pat`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)

  uint64_t k = gid * (uint64_t)Q + slot;              // a group's Q patterns are neighbours: their offsets,
  const uint64_t kstride = ngroups * (uint64_t)Q;     // symbols and outputs share cache lines
  bool active = k < npat, fresh = true;
  uint64_t pbeg = 0;
  uint32_t j = 0, s = 0, e = 0, c = 0, nsteps = 0;
  while (__any(active)) {
    if (active && fresh) {
      pbeg = off[k];
      const uint64_t pend = off[k + 1];
      j = (uint32_t)(pend - pbeg);
      // offsets that go backwards or leave the pattern buffer: refuse, do not read (j = 0 from here on)
      const bool badoff = FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
      if (badoff) j = 0;
      bool bad = badoff;
      if (s0e0) {              // Search::search on an existing Search (wrapper.rs:105-106)
        const uint64_t s64 = s0e0[2 * k], e64 = s0e0[2 * k + 1];
        s = (uint32_t)s64;
        e = (uint32_t)e64;
        if (s64 > n || e64 > n || badoff) {            // not a range of this index: refuse, do not read
          bad = true;
          s = 0; e = 0; j = 0;
        }
      } else {                 // (0, len)   wrapper.rs:41
        s = 0;
        e = badoff ? 0u : n;
      }
      if (bad && owner) atomicOr(status, 1u << FMX_ERR_ARG);
      c = j ? pat[pbeg + j - 1] : 0u;                  // last symbol: pattern.iter().rev()
      fresh = false;
    }
    const bool stepping = active && j != 0 && c <= max_character;
    // the next symbol rides along with this round's record loads
    uint32_t cn = 0;
    if (stepping && j > 1) cn = pat[pbeg + j - 2];
    const uint32_t sx = stepping ? s : NONE;
    const unsigned long long wm = __ballot(stepping);
    uint4 a[Q], b[Q];
    uint32_t sq[Q], eq[Q], cq[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
      sq[q] = NONE; eq[q] = 0; cq[q] = 0;
      if (!(wm & (SLOT0 << q))) continue;              // pattern q idle in every group of the wave
      sq[q] = fmx_slot_bcast<Q>(sx, q);
      eq[q] = fmx_slot_bcast<Q>(e, q);
      cq[q] = fmx_slot_bcast<Q>(c, q);
      if (sq[q] != NONE) {                             // group-uniform
        const uint32_t rs = sq[q] >> 8, re = eq[q] >> 8;
        FMX_CHECK(rs < nrec && re < nrec);
        FMX_TOUCH_G0(g, &rec[(size_t)rs * 8u]);
        if (re != rs) FMX_TOUCH_G0(g, &rec[(size_t)re * 8u]);   // both ends in one record: ONE line
        a[q] = rec[(size_t)rs * 8u + g];
        b[q] = rec[(size_t)re * 8u + g];
      }
    }
#pragma unroll
    for (int q = 0; q < Q; q++) {
      if (!(wm & (SLOT0 << q))) continue;
      if (sq[q] != NONE) {
        const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(a[q], sq[q] & 255u, cq[q], g));  // wrapper.rs:109
        const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(b[q], eq[q] & 255u, cq[q], g));  // wrapper.rs:110
        if (slot == (uint32_t)q) { s = ns; e = ne; }
      }
    }
    if (active) {
      bool done = j == 0;
      if (!done) {
        if (!stepping) {                               // reference: panic on cs[c]
          if (owner) atomicOr(status, 1u << FMX_ERR_SYMBOL_RANGE);
          s = 0; e = 0; done = true;
        } else {
          c = cn;
          j--;
          nsteps++;
          if (s == e || j == 0) done = true;           // wrapper.rs:111-113
        }
      }
      if (done) {
        if (owner) {
          if (out_s) out_s[k] = s;
          if (out_e) out_e[k] = e;
          if (out_cnt) out_cnt[k] = (uint64_t)(e - s);  // wrapper.rs:132-134
        }
        k += kstride;
        active = k < npat;
        fresh = true;
      }
    }
  }
  if (steps_out && owner && nsteps)
    atomicAdd((unsigned long long *)steps_out, (unsigned long long)nsteps);
}


// ---------------------------------------------------------------------------
// Alternatives to the 8-lane-group shape (DESIGN.md section 4.1 table; FMX_VARIANT=8 / 9):
//   fmx_count_f3_lane_kernel  -- one LANE owns one pattern and reads both 128-B records itself
//                                (8 dwordx4 loads per record, no cross-lane traffic)
//   fmx_count_f3_wave_kernel  -- one WAVEFRONT owns one pattern (lanes 0-7 fetch the record of s,
//                                lanes 8-15 the record of e, the other 48 lanes idle)
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// Measurement-only alternatives to the 8-lane-group shape (DESIGN.md section 4.1 table; selected
// with FMX_VARIANT=8 / 9, never used by default):
//   fmx_count_f3_lane_kernel  -- one LANE owns one pattern and reads both 128-B records itself
//                                (8 dwordx4 loads per record, no cross-lane traffic)
//   fmx_count_f3_wave_kernel  -- one WAVEFRONT owns one pattern (lanes 0-7 fetch the record of s,
//                                lanes 8-15 the record of e, the other 48 lanes idle)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fmx_rank_whole_record(const uint4 *__restrict__ r, uint32_t off,
                                                          uint32_t c) {
  uint32_t acc = r[c].x;  // absolute counter of symbol c
#pragma unroll
  for (uint32_t g = 0; g < 8; g++) {
    const uint4 p = r[g];
    int nb = (int)off - (int)(g * 32);
    nb = nb < 0 ? 0 : (nb > 32 ? 32 : nb);
    acc += __popc(fmx_piece_match<3>(p, c) & (uint32_t)((1ull << nb) - 1ull));
  }
  return acc;
}
__global__ __launch_bounds__(FMX_BLOCK) void fmx_count_f3_lane_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character, uint32_t *status,
    const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_cnt,
    uint64_t *__restrict__ steps_out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint32_t nsteps = 0;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < npat; k += stride) {
    const uint64_t pbeg = off[k];
    uint32_t j = (uint32_t)(off[k + 1] - pbeg), s = 0, e = n;
    while (j) {
      nsteps++;
      const uint32_t c = pat[pbeg + --j];
      if (c > max_character) { atomicOr(status, 1u << FMX_ERR_SYMBOL_RANGE); s = e = 0; break; }
      s = fmx_rank_whole_record(rec + (size_t)(s >> 8) * 8u, s & 255u, c);
      e = fmx_rank_whole_record(rec + (size_t)(e >> 8) * 8u, e & 255u, c);
      if (s == e) break;
    }
    if (out_s) out_s[k] = s;
    if (out_e) out_e[k] = e;
    if (out_cnt) out_cnt[k] = (uint64_t)(e - s);
  }
  if (steps_out && nsteps) atomicAdd((unsigned long long *)steps_out, (unsigned long long)nsteps);
}
__global__ __launch_bounds__(FMX_BLOCK) void fmx_count_f3_wave_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character, uint32_t *status,
    const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_cnt,
    uint64_t *__restrict__ steps_out) {
  const uint32_t lane = threadIdx.x & 63u, g = lane & 7u;
  if (lane >= 16u) return;                 // 48 of the 64 lanes have nothing to fetch
  const bool is_e = lane >= 8u;
  const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  uint32_t nsteps = 0;
  for (uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; k < npat; k += nwaves) {
    const uint64_t pbeg = off[k];
    uint32_t j = (uint32_t)(off[k + 1] - pbeg);
    uint32_t v = is_e ? n : 0u;            // lanes 0-7 carry s, lanes 8-15 carry e
    bool dead = false;
    while (j && !dead) {
      const uint32_t c = pat[pbeg + --j];
      if (c > max_character) { if (lane == 0) atomicOr(status, 1u << FMX_ERR_SYMBOL_RANGE); v = 0; break; }
      const uint4 p = rec[(size_t)(v >> 8) * 8u + g];
      v = fmx_group_sum(fmx_piece_rank<3>(p, v & 255u, c, g));
      const uint32_t other = (uint32_t)__shfl((int)v, (int)(lane ^ 8u));
      dead = (v == other);
      nsteps++;
    }
    if (g == 0) {
      if (!is_e && out_s) out_s[k] = v;
      if (is_e && out_e) out_e[k] = v;
    }
    const uint32_t sv = (uint32_t)__shfl((int)v, (int)(lane & 7u));
    if (lane == 8 && out_cnt) out_cnt[k] = (uint64_t)(v - sv);
  }
  if (steps_out && lane == 0 && nsteps) atomicAdd((unsigned long long *)steps_out, (unsigned long long)nsteps);
}


// the round-1/2 form of the DNA walk, kept for A/B runs (FMX_VARIANT=22)
// locate walk, single 3-bit level (DNA).  The wave's 8 groups take hits from the queue above as they
// finish (ballot + prefix popcount), so the wave runs sum(work) / (8 Q) iterations, not max over its
// groups; a finishing group takes its next row from the register window with a ds_bpermute -- no
// dependent memory access to start a walk.  Every iteration a group issues exactly ONE 16-B load per
// lane whose address depends on its state -- a record piece while walking (fm_index.rs:134-137) or
// the aligned chunk holding its SA sample once the row is sampled (sample.rs:46-60) -- so walking
// and finishing groups of one wave overlap their latencies instead of serialising two branches.
// TEXT: text-order sampling (FmxDev::phase).  A walk is then four kinds of iteration, each ONE 16-byte
// load per lane like before: read the row's phase piece -> `phase` LF steps (no test in between) ->
// read the final row's phase piece for its rank among the sampled rows -> read the sample.
template <int Q, bool TEXT>
__global__ __launch_bounds__(FMX_LOC_BLOCK) void fmx_locate_f3w_kernel(
    const uint4 *__restrict__ rec, const uint32_t *__restrict__ samples, const uint4 *__restrict__ phase,
    uint32_t n, uint32_t sa_level, uint64_t total, uint32_t hits_per_block, uint32_t chunk,
    const uint32_t *__restrict__ rows, uint64_t *__restrict__ out_pos, uint64_t *__restrict__ steps_out) {
  __shared__ unsigned int lds_q;
  if (threadIdx.x == 0) lds_q = 0;
  __syncthreads();
  const uint64_t blo = (uint64_t)blockIdx.x * hits_per_block;
  if (blo >= total) return;                           // block-uniform
  const uint32_t bn = (uint32_t)(total - blo < hits_per_block ? total - blo : hits_per_block);
  // Q independent walks per group: Q record loads in flight per lane (the longest single walk of
  // the batch still bounds the kernel from below).
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = lane & (FMX_GROUP - 1);
  const uint32_t grp = lane >> 3;
  const uint32_t lmask = (1u << sa_level) - 1u;
  const uint4 *samp4 = reinterpret_cast<const uint4 *>(samples);
  FmxHitQueue<> hq;
  hq.init(rows + blo, blo, bn, chunk, lane, lds_q);

  uint64_t h[Q], pend_h[Q], pend_v[Q];
  uint32_t row[Q], steps[Q];
  // TEXT: stage of the walk (0 phase of the start row, 1 LF steps, 2 rank at the final row, 3 sample),
  // LF steps still to do, index of the sample
  [[maybe_unused]] uint32_t st[Q], rem[Q], sidx[Q];
  bool active[Q], pending[Q];
  uint32_t nsteps = 0;
#pragma unroll
  for (int q = 0; q < Q; q++) {
    active[q] = hq.take(grp, h[q], row[q]);
    hq.advance(8u, lds_q);
    if (!active[q]) row[q] = 0u;
    steps[q] = 0;
    st[q] = 0; rem[q] = 0; sidx[q] = 0;
    pending[q] = false;
    pend_h[q] = 0;
    pend_v[q] = 0;
  }
  for (;;) {
    // slots that are dead in EVERY group of the wave are skipped altogether (wave-uniform): towards
    // the end of a batch a wave holds one or two long walks, and an iteration then costs one
    // slot's instructions instead of Q slots' -- the tail runs at memory latency, not at issue rate
    bool live[Q];
    bool any = false;
#pragma unroll
    for (int q = 0; q < Q; q++) {
      live[q] = __any(active[q]) != 0;
      any |= live[q] || __any(pending[q]) != 0;
    }
    if (!any) break;
    // issue every load of this round
    uint4 p[Q];
    bool sampled[Q];
    [[maybe_unused]] uint32_t pt[Q];               // TEXT: the row's index inside its phase piece
#pragma unroll
    for (int q = 0; q < Q; q++) {
      sampled[q] = TEXT ? st[q] == 3u : (row[q] & lmask) == 0;
      p[q] = make_uint4(0u, 0u, 0u, 0u);
      pt[q] = 0;
      if (live[q] && active[q]) {
        const uint32_t si = TEXT ? sidx[q] : row[q] >> sa_level;
        FMX_CHECK(row[q] < n && (row[q] >> 8) < n / 256u + 1u);
        FMX_CHECK(!sampled[q] || (uint64_t)si <= (((uint64_t)n - 1) >> sa_level));
        const uint4 *addr = sampled[q] ? (samp4 + (si >> 2)) : (rec + ((size_t)(row[q] >> 8) * 8u + g));
        if (TEXT && (st[q] == 0u || st[q] == 2u)) addr = phase + fmx_phase_piece(row[q], sa_level, pt[q]);
        FMX_TOUCH_G0(g, (!TEXT || st[q] == 1u) && !sampled[q] ? addr - g : addr);
        p[q] = *addr;
      }
    }
    // positions finished in the previous round are stored behind these loads
#pragma unroll
    for (int q = 0; q < Q; q++) {
      if (pending[q] && g == 0) out_pos[pend_h[q]] = pend_v[q];
      pending[q] = false;
    }
#pragma unroll
    for (int q = 0; q < Q; q++) {
      if (!live[q]) continue;                                     // wave-uniform
      bool fin = false;
      if (active[q]) {
        if (sampled[q]) {
          const uint32_t w = (TEXT ? sidx[q] : row[q] >> sa_level) & 3u;
          const uint32_t p0 = p[q].x, p1 = p[q].y, p2 = p[q].z, p3 = p[q].w;
          const uint32_t sa = w == 0 ? p0 : (w == 1 ? p1 : (w == 2 ? p2 : p3));
          uint64_t v = (uint64_t)sa + steps[q];     // fm_index.rs:131-133: (sa + steps) % len
          if (v >= n) v -= n;
          pend_v[q] = v;
          pend_h[q] = h[q];
          pending[q] = true;
          fin = true;
        } else if (TEXT && st[q] != 1u) {           // phase piece: of the start row (0) or the final row (2)
          uint32_t rank0;
          const uint32_t phi = fmx_phase_decode(p[q], pt[q], sa_level, rank0);
          sidx[q] = rank0;
          rem[q] = phi;
          st[q] = (st[q] == 2u || phi == 0u) ? 3u : 1u;
        } else {
          const uint32_t off = row[q] & 255u;
          const uint32_t sym =
              fmx_group_sum((g == (off >> 5)) ? fmx_piece_code<3>(p[q], off & 31u) : 0u);
          row[q] = fmx_group_sum(fmx_piece_rank<3>(p[q], off, sym, g));  // lf_map (absolute counters)
          steps[q]++;
          nsteps++;
          if (TEXT && --rem[q] == 0u) st[q] = 2u;
        }
      }
      const unsigned long long fmask = __ballot(fin && g == 0);  // one bit per finishing group
      if (fmask) {                                                // wave-uniform
        const uint32_t leader = lane & ~7u;
        const uint32_t my_rank = (uint32_t)__popcll(fmask & ((1ull << leader) - 1ull));
        uint64_t h_new;
        uint32_t r_new;
        const bool ok = hq.take(my_rank, h_new, r_new);
        if (fin) {
          h[q] = h_new;
          active[q] = ok;
          row[q] = ok ? r_new : 0u;
          steps[q] = 0;
          st[q] = 0;
        }
        hq.advance((uint32_t)__popcll(fmask), lds_q);
      }
    }
  }
  if (steps_out && g == 0 && nsteps)
    atomicAdd((unsigned long long *)steps_out, (unsigned long long)nsteps);
}

// count: returns true when an alternative kernel was launched
static bool fmx_measure_count(const FmxCountCall &c, const FmxTune &tn, const FmxRoute &r) {
  const fmx_index *idx = c.idx;
  const FmxMwm &w = c.dv.bw;
  const bool dna = idx->kind == FMX_KIND_FM && idx->sym_bytes == 1 && w.nlevels == 1 && w.lv[0].fmt == 3;
  const bool pair = c.dv.pair_rec && idx->sym_bytes == 1 && tn.use_pair;
  const int sm = fmx_select_mode(idx, c.dv);
  switch (tn.alt) {
    case 100:  // generic kernels everywhere; RLFM per select structure (instantiations only these builds have)
      if (idx->kind == FMX_KIND_RLFM && sm == 1) { fmx_route_nl_km<FMX_KIND_RLFM, 1>(r, fmx_count_group(c)); return true; }
      if (idx->kind == FMX_KIND_RLFM && sm == 2) { fmx_route_nl_km<FMX_KIND_RLFM, 2>(r, fmx_count_group(c)); return true; }
      return false;                                  // tn.generic steers the shipped dispatch
    case 20:   // endpoint per lane on an FM index
      if (idx->kind != FMX_KIND_FM || pair) return false;
      fmx_route_nl_km<FMX_KIND_FM, 0>(r, fmx_count_ep(c, fmx_ep_count_blocks(c.npat, tn.ep_blocks)));
      return true;
    default: break;
  }
  if (!dna || pair) return false;
#define FMX_F3D_LAUNCH(Q)                                                                          \
  hipLaunchKernelGGL((fmx_count_f3d_kernel<Q>), dim3(fmx_grid_for_groups((c.npat + Q - 1) / Q)),     \
                     dim3(FMX_BLOCK), 0, c.st, w.lv[0].rec, c.dv.n, c.dv.max_character, c.dv.status,  \
                     (const uint8_t *)c.pat, c.off, c.npat, c.s0e0, c.s, c.e, c.cnt, c.steps)
  switch (tn.alt) {
    case 8:  // lane per pattern
      if (c.s0e0) return false;
      hipLaunchKernelGGL(fmx_count_f3_lane_kernel, dim3(FMX_MAX_BLOCKS), dim3(FMX_BLOCK), 0, c.st, w.lv[0].rec,
                         c.dv.n, c.dv.max_character, c.dv.status, (const uint8_t *)c.pat, c.off, c.npat, c.s, c.e,
                         c.cnt, c.steps);
      return true;
    case 9:  // wavefront per pattern
      if (c.s0e0) return false;
      hipLaunchKernelGGL(fmx_count_f3_wave_kernel, dim3(FMX_MAX_BLOCKS), dim3(FMX_BLOCK), 0, c.st, w.lv[0].rec,
                         c.dv.n, c.dv.max_character, c.dv.status, (const uint8_t *)c.pat, c.off, c.npat, c.s, c.e,
                         c.cnt, c.steps);
      return true;
    case 2: FMX_F3_LAUNCH(c, 2, false, false); return true;
    case 3: FMX_F3_LAUNCH(c, 1, true, false); return true;
    case 4: FMX_F3_LAUNCH(c, 2, true, false); return true;
    case 5: FMX_F3_LAUNCH(c, 4, false, false); return true;
    case 24: FMX_F3D_LAUNCH(4); return true;
    case 25: FMX_F3D_LAUNCH(2); return true;
    default: return false;
  }
}

// locate: returns true when an alternative kernel was launched
static bool fmx_measure_locate(const FmxLocateCall &c, const FmxTune &tn, int sm) {
  (void)sm;
  const fmx_index *idx = c.idx;
  const FmxMwm &w = c.dv.bw;
  const bool dna = idx->kind == FMX_KIND_FM && w.nlevels == 1 && w.lv[0].fmt == 3;
  if (!dna) return false;
  if (tn.alt == 21) {          // one walk per lane on the one-level index
    const bool big = c.total >= (4u << 20);
    const unsigned thr = tn.ep_loc_threads ? (unsigned)tn.ep_loc_threads : (big ? 640u : (unsigned)FMX_LOC_BLOCK);
    uint32_t hpb;
    unsigned gr;
    c.slice(tn.ep_loc_blocks ? (uint64_t)tn.ep_loc_blocks : (big ? 512 : 256), FMX_LCHUNK, hpb, gr);
    FMX_EPL_SM(c, gr, thr, hpb, tn.wc, FMX_KIND_FM, 0);
    return true;
  }
  if (tn.alt != 22 && tn.alt != 23 && tn.alt != 15) return false;
  const int q = tn.walks ? tn.walks : (c.total >= (1u << 16) ? 4 : 1);
  const unsigned lthreads = (unsigned)tn.loc_threads;
  const uint64_t nb = tn.loc_blocks ? (uint64_t)tn.loc_blocks : (c.total >= (4u << 20) && tn.alt != 22 ? 512 : 256);
  const uint64_t per_wave = (c.total + nb * (lthreads / 64) - 1) / (nb * (lthreads / 64));
  uint32_t chunk = (uint32_t)((per_wave + 7) / 8 * 8);
  if (chunk < 8u * (uint32_t)q) chunk = 8u * (uint32_t)q;
  if (chunk > FMX_LCHUNK) chunk = FMX_LCHUNK;
  uint32_t hpb;
  unsigned gr;
  c.slice(nb, chunk, hpb, gr);
#define FMX_LOC_LAUNCH(Q, TEXT)                                                                    \
  hipLaunchKernelGGL((fmx_locate_f3w_kernel<Q, TEXT>), dim3(gr), dim3(FMX_LOC_BLOCK), 0, c.st,        \
                     w.lv[0].rec, c.dv.samples, c.dv.phase, c.dv.n, c.dv.sa_level, c.total, hpb, chunk, \
                     c.rows, c.pos, c.steps)
  if (tn.alt == 22) {          // walk state repeated in all 8 lanes
    if (c.dv.phase) { if (q == 4) FMX_LOC_LAUNCH(4, true); else if (q == 2) FMX_LOC_LAUNCH(2, true); else FMX_LOC_LAUNCH(1, true); }
    else { if (q == 4) FMX_LOC_LAUNCH(4, false); else if (q == 2) FMX_LOC_LAUNCH(2, false); else FMX_LOC_LAUNCH(1, false); }
    return true;
  }
  if (c.dv.phase) return false;
  if (tn.alt == 23) {          // distributed state, hand-over at the end of the round
    if (q == 4) FMX_LOCQ_LAUNCH(c, gr, lthreads, hpb, chunk, 4, false);
    else if (q == 2) FMX_LOCQ_LAUNCH(c, gr, lthreads, hpb, chunk, 2, false);
    else FMX_LOCQ_LAUNCH(c, gr, lthreads, hpb, chunk, 1, false);
    return true;
  }
  // 15: 8 walks per group (16 % fewer instructions per walk, 71 VGPRs, no faster)
  if (chunk == FMX_LCHUNK && tn.wc) FMX_LOCP_LAUNCH(c, gr, lthreads, hpb, chunk, 8, true);
  else FMX_LOCP_LAUNCH(c, gr, lthreads, hpb, chunk, 8, false);
  return true;
}
