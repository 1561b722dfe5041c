// mh_nn_flat.h -- the plan / scan matcher (round 5): the bounded correspondence search of a large layer with the
// per-point bookkeeping done ONCE per point, the per-voxel work once per candidate voxel and the per-record work once
// per record -- each at 64 work items per wave -- and the three kinds of work item handed from one phase to the next
// through the wave's slice of LDS.
//
// Why: the quad matcher (nn_search_quad, mh_nn_device.h) gives a point four lanes, and every lane of the quad repeats the
// point's bookkeeping -- fp64 transform, voxel index, slab gaps, 27 lower bounds, batch selection, key / hash / resolve /
// narrow of the probed voxel, merged-range selects: ~750 vector instructions per wave of SIXTEEN points of which ~100 test
// records (profiles/r04_match_kernel.md, VERDICT r4 "what's weak" 3).  Here a wave owns 64 consecutive scan points:
//   A1  lane = point      load l and the previous pairing, p' = (float)(R l + t), bound b0 = d2(p', old partner), voxel,
//                         gaps, the 27 lower bounds -> bit mask of candidate voxels (every voxel that can hold a record within
//                         b0: the own voxel and, for a converging alignment, 1-7 neighbours); the (point, code) pairs of the
//                         wave are written to LDS back to back (DPP prefix sum of the popcounts);
//   A2  lane = candidate  key, hash, ONE probe per lane, resolve, narrow to the hull of the quadrants of the sub-voxel
//                         index that can hold a record within b0 (quad_narrow) -> the range is cut into chunks of <= 4
//                         consecutive records, written to LDS back to back (second prefix sum);
//   B   lane = record     lane 4c+s tests record s of chunk c: d2 in the candidate arithmetic, key (d2 bits << 32 | scan
//                         position), ds_min_u64 into the point's result word (LDS atomic: the minimum does not depend on
//                         the order) -- no lane waits for a neighbour's longer list, no DPP reduction, W chunks per lane in
//                         flight;
//   C   lane = point      the winner's record from `pts`, threshold test, pairing stored (coalesced: 16 + 4 bytes per lane);
//   D   quad = point      the points the plan does not cover run nn_search_quad as before, sixteen at a time off a compacted
//                         list (ballot + prefix count): no previous pairing (ICP iteration 0: all of them), more than
//                         kFlatMaxCand candidate voxels, chunk space exhausted, or the bound not attained inside the 27-voxel
//                         block (the old partner left it: nothing beat the initial key -> once more without a bound).
// Exactness: the result of the reference's scan is the lexicographic minimum of (d2, scan position) over the 27-voxel block.
// b0 is attained by a map record, so whenever that record lies in the block the minimum has d2 <= b0; the candidate voxels
// are every voxel whose conservative lower bound does not exceed b0 and quad_narrow only drops quadrants whose every record
// is provably farther than b0 -- the set of tested records contains every record of the block with d2 <= b0, and the minimum
// over it is the block's.  Same fp32 arithmetic, same 64-bit key as nn_scan_round_quad: bit-identical pairings
// (tests/test_gpu_parity.py, tests/test_gpu_fullsize.py, tools/fuzz_bound.py with MH_MATCH=f).
#pragma once
#include "mh_nn_device.h"

namespace mh {

constexpr int kFlatLPP = 4;            // records per chunk = lanes per chunk (consecutive 16-byte records: one L1 line mostly)
#ifndef MH_FLAT_W
#define MH_FLAT_W 8
#endif
#ifndef MH_FLAT_PROBES
#define MH_FLAT_PROBES 4
#endif
constexpr int kFlatProbes = MH_FLAT_PROBES;  // probes in flight per lane (passes of 64 candidate voxels resolved per round trip)
constexpr int kFlatW = MH_FLAT_W;      // chunks in flight per lane group and round: 16 x W chunks per wave and round trip
constexpr int kFlatMaxCand = 8;        // candidate voxels per point on the planned path (C2: 99.9 % of the points have <= 8)
#ifndef MH_FLAT_CHUNKS
#define MH_FLAT_CHUNKS 768
#endif
constexpr int kFlatMaxChunks = MH_FLAT_CHUNKS;  // per wave (C2: ~320)
constexpr uint32_t kFlatMaxRecords = 1u << 30;  // chunk word = first record (30 bits) | (records - 1) << 30

// MAXC: candidate voxels per point on the planned path; NCL: entries of the candidate list (>= points per wave x MAXC);
// NCH: entries of the chunk list.
template <int MAXC, int NCL, int NCH>
struct FlatWaveT {
  static constexpr int kMaxCand = MAXC;
  static constexpr int kCands = NCL;
  static constexpr int kMaxChunks = NCH;
  f32x4 P[64];                         // p' and the bound b0 (phase D: the bound the quad search is to start from)
  unsigned long long KB[64];           // packed key of voxel (cx-1, cy-1, cz-1)
  unsigned long long RES[64];          // best (d2 bits << 32 | scan position) so far, ds_min_u64
  uint32_t CH[NCH];                    // chunk: first record | (records - 1) << 30
  unsigned short CL[NCL];              // candidate: point | code << 8
  unsigned char CHP[NCH];              // the chunk's point
  unsigned char SLOWF[64];             // the plan ran out of chunk space for this point
  unsigned char SL[64];                // phase D: the points to search quad-wise, compacted
  uint32_t NCH_, NVALID;               // chunks allocated (ds_add_rtn); first chunk slot that was not written (ds_min)
};
typedef FlatWaveT<kFlatMaxCand, 64 * kFlatMaxCand, kFlatMaxChunks> FlatWave;   // the large layers' matcher (k_match_flat*): C2 shapes
#ifndef MH_LW_NCL
#define MH_LW_NCL 1024
#endif
#ifndef MH_LW_NCH
#define MH_LW_NCH 1024
#endif
typedef FlatWaveT<27, MH_LW_NCL, MH_LW_NCH> FlatWaveSmall;  // the small layer's loop (k_icpw): <= 37 points per wave, every candidate count planned

// count of set bits of `m` below this lane
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Phases A2 and B for one set of candidate masks (mh_nn_flat.h's header): the wave's (point, code) pairs to LDS, a probe per
// pair, the narrowed ranges cut into chunks, a lane per record of every chunk.  `init`: what a point's result word starts from
// (the bound and "no record", or what an earlier stage found).  Returns the number of candidate pairs (wave-uniform); with none,
// nothing is written to LDS.  `ins`: what phase B does with the key of a record within the bound -- the minimum into the point's
// result word here, the k smallest into k words for pairingsPerPoint > 1 (mh_k_match_kbest.h).
struct FlatInsertMin {
  template <class FW>
  __device__ __forceinline__ void operator()(FW& sh, uint32_t p, unsigned long long key) const {
    (void)__hip_atomic_fetch_min(&sh.RES[p], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};
// OFF32: 32-bit byte offsets on scalar bases for the probes and the record loads (gat, mh_nn_device.h); the default is the code every
// other caller keeps.
template <bool OFF32 = false, class FW, class INS = FlatInsertMin>
__device__ __forceinline__ uint32_t flat_plan_scan(FW& sh, const MapView& m, uint32_t lane, uint32_t cmask, unsigned long long kbase,
                                                   float px, float py, float pz, float b0, unsigned long long init,
                                                   const INS ins = INS()) {
  constexpr int kFlatMaxCand = FW::kMaxCand;
  constexpr int kFlatMaxChunks = FW::kMaxChunks;
  const gslots_ptr slots4 = (gslots_ptr)m.slots;
  const gpts_ptr spts = (gpts_ptr)m.pts_q;
  uint32_t n_cands;
  const uint32_t ncand = (uint32_t)__builtin_popcount(cmask);
  const uint32_t cincl = wave_scan_incl(ncand);
  n_cands = (uint32_t)__builtin_amdgcn_readlane((int)cincl, 63);
  sh.P[lane] = (f32x4){px, py, pz, b0};
  uint32_t nvalid = 0;  // chunks written (wave-uniform)
  if (n_cands) {        // wave-uniform
    sh.KB[lane] = kbase;
    sh.RES[lane] = init;
    sh.SLOWF[lane] = 0;
    if (lane == 0) { sh.NCH_ = 0; sh.NVALID = (uint32_t)kFlatMaxChunks; }
    {
      uint32_t mm = cmask, at = cincl - ncand;
      if (kFlatMaxCand <= 8) {
#pragma unroll
        for (int j = 0; j < (kFlatMaxCand <= 8 ? kFlatMaxCand : 1); j++) {
          if (mm) {
            const uint32_t code = (uint32_t)__builtin_ctz(mm);
            mm &= mm - 1;
            sh.CL[at + (uint32_t)j] = (unsigned short)(lane | (code << 8));
          }
        }
      } else {
        while (mm) {  // (up to 27 codes: a loop as long as the wave's longest list)
          const uint32_t code = (uint32_t)__builtin_ctz(mm);
          mm &= mm - 1;
          sh.CL[at++] = (unsigned short)(lane | (code << 8));
        }
      }
    }
    wave_sync_lds_nn();
    // ---- A2: the candidate voxel ---------------------------------------------------------------------------------------
    // kFlatProbes passes of 64 candidates at a time: every lane's probes are in flight together (one round trip for the
    // wave's first 256 candidates -- C2: ~207), then resolved one after the other.
    uint32_t nch_total = 0;  // (wave-uniform)
    for (uint32_t base = 0; base < n_cands; base += 64u * (uint32_t)kFlatProbes) {
      uint32_t ent[kFlatProbes];
      unsigned long long keys[kFlatProbes];
      u32x4 sls[kFlatProbes];
#pragma unroll
      for (int k = 0; k < kFlatProbes; k++) {
        const uint32_t c = base + 64u * (uint32_t)k + lane;
        ent[k] = sh.CL[c < n_cands ? c : 0u];  // (clamped: the load of an idle lane is a hit on entry 0's slot)
        keys[k] = nn_key_of(sh.KB[ent[k] & 63u], (int)(ent[k] >> 8));
        sls[k] = *gat<OFF32>(slots4, hash_key(keys[k]) & m.mask);
      }
#pragma unroll
      for (int k = 0; k < kFlatProbes; k++) {
        if (base + 64u * (uint32_t)k >= n_cands) break;  // wave-uniform
        const uint32_t c = base + 64u * (uint32_t)k + lane;
        const bool act = c < n_cands;
        const uint32_t p = ent[k] & 63u;
        const int code = (int)(ent[k] >> 8);
        const f32x4 P = sh.P[p];
        uint32_t f, cnt, qv;
        nn_resolve<OFF32>(m, slots4, keys[k], sls[k], act, f, cnt, &qv);
        quad_narrow(m, qv, code, P.x, P.y, P.w, f, cnt);
        const uint32_t nchunks = (cnt + (uint32_t)kFlatLPP - 1u) / (uint32_t)kFlatLPP;
        // chunk space by a DPP prefix sum over the wave's candidates of this pass (the order of the chunks does not matter
        // for the result: every chunk names its point)
        const uint32_t incl = wave_scan_incl(nchunks);
        const uint32_t pos = nch_total + incl - nchunks;
        nch_total += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (nchunks) {
          if (pos + nchunks > (uint32_t)kFlatMaxChunks) {  // out of space: the point goes to phase D, slots from `pos` on stay unwritten
            sh.SLOWF[p] = 1;
            (void)__hip_atomic_fetch_min(&sh.NVALID, pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          } else {
#pragma unroll 1
            for (uint32_t j = 0; j < nchunks; j++) {
              const uint32_t rem = cnt - (uint32_t)kFlatLPP * j;
              sh.CH[pos + j] = (f + (uint32_t)kFlatLPP * j) | (((rem < (uint32_t)kFlatLPP ? rem : (uint32_t)kFlatLPP) - 1u) << 30);
              sh.CHP[pos + j] = (unsigned char)p;
            }
          }
        }
      }
    }
    wave_sync_lds_nn();
    {
      const uint32_t a = nch_total;
      const uint32_t b = sh.NVALID;
      nvalid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(a < b ? a : b));
    }
    // ---- B: the record ---------------------------------------------------------------------------------------------------
    const uint32_t grp = lane >> 2, sub = lane & 3u;
    for (uint32_t t0 = 0; t0 < nvalid; t0 += 16u * (uint32_t)kFlatW) {
      f32x4 rec[kFlatW];
      uint32_t pp[kFlatW];
      bool valid[kFlatW];
#pragma unroll
      for (int u = 0; u < kFlatW; u++) {
        const uint32_t t = t0 + 16u * (uint32_t)u + grp;
        const bool ok = t < nvalid;
        const uint32_t tt = ok ? t : 0u;  // (chunk 0 exists: nvalid > 0)
        const uint32_t ch = sh.CH[tt];
        pp[u] = sh.CHP[tt];
        const uint32_t last = ch >> 30;
        valid[u] = ok && sub <= last;
        rec[u] = *gat<OFF32>(spts, (ch & 0x3FFFFFFFu) + (sub < last ? sub : last));  // clamped into the chunk: no load behind a branch
      }
#pragma unroll
      for (int u = 0; u < kFlatW; u++) {
        const f32x4 Pq = sh.P[pp[u]];  // (read when the record is there: W records in flight cost 4 registers each, not 8)
        const float dx = rec[u].x - Pq.x, dy = rec[u].y - Pq.y, dz = rec[u].z - Pq.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;  // fp32, un-fused, this order (bit-exact with the oracle)
        // only a record within the bound can be the answer ((d2, position) < (b0, none) <=> d2 <= b0)
        if (valid[u] && d2 <= Pq.w) ins(sh, pp[u], ((unsigned long long)__float_as_uint(d2) << 32) | __float_as_uint(rec[u].w));
      }
    }
    wave_sync_lds_nn();
  }
  return n_cands;
}

// One wave, 64 consecutive scan points starting at `i0` (lanes past `n` idle).  Everything uniform (pose, thresholds,
// have_prev) comes in SGPRs.
// The pairing's fourth word: d2 of the nearest record, its SIGN the verdict of the distance test (set = not accepted; d2 >= 0, so
// the bit is free) -- the accumulation that follows this matcher (k_accum<true>) then needs the 16 bytes of the pairing and not
// the 4 of the index array as well: 28 instead of 32 bytes per point of a launch that streams at 0.57 of the HBM peak.  The index
// array is still written (covariance, final pairings); whoever reads the distance takes its absolute value.
__device__ __forceinline__ float flat_signed_d2(float d2, bool accepted) {
  return __uint_as_float(__float_as_uint(d2) | (accepted ? 0u : 0x80000000u));
}
// OFF32: every byte offset into the slot table, both record arrays and the scan's arrays fits 32 bits (the host's flat_off32): they
// are formed in 32 bits on scalar bases (gat, mh_nn_device.h).
template <bool OFF32 = false>
__device__ __forceinline__ void match_flat_wave(FlatWave& sh, const MapView& m, const double* __restrict__ T, float thr2,
                                                float ang2, bool have_prev, const float* __restrict__ lx,
                                                const float* __restrict__ ly, const float* __restrict__ lz, uint32_t n,
                                                uint32_t i0, float4* __restrict__ pair_q, uint32_t* __restrict__ pair_gidx) {
  const uint32_t lane = (uint32_t)__lane_id();
  const uint32_t i = i0 + lane;
  const bool in = i < n;
  const uint32_t ic = in ? i : n - 1;
  const gslots_ptr slots4 = (gslots_ptr)m.slots;
  const gpts_ptr pts4 = (gpts_ptr)m.pts;
  const gpts_ptr spts = (gpts_ptr)m.pts_q;
  // ---- A1: the point ------------------------------------------------------------------------------------------------
  const float x = *gat<OFF32>(G(lx), ic), y = *gat<OFF32>(G(ly), ic), z = *gat<OFF32>(G(lz), ic);
  f32x4 prev = (f32x4){0.f, 0.f, 0.f, __builtin_inff()};
  if (have_prev) prev = *gat<OFF32>(G(reinterpret_cast<const f32x4*>(pair_q)), ic);  // grid-uniform branch
  float px, py, pz;
  transform_point(T, x, y, z, px, py, pz);
  float b0 = __builtin_inff();
  if (fabsf(prev.w) < __builtin_inff()) {  // (the sign is the verdict: flat_signed_d2)
    const float dx = prev.x - px, dy = prev.y - py, dz = prev.z - pz;
    b0 = (dx * dx + dy * dy) + dz * dz;  // the candidate arithmetic
  }
  const float lim = 1.0e6f;
  const bool okrange = ((int)(fabsf(px * m.inv_vs) < lim) & (int)(fabsf(py * m.inv_vs) < lim) & (int)(fabsf(pz * m.inv_vs) < lim)) != 0;
  // Points WITHOUT a bound (ICP iteration 0; a point whose old partner was not found) get one first: stage 0 plans and scans
  // their OWN voxel only -- what the quad search does first, but as lane-per-record work -- and the nearest record of it, if
  // there is one, bounds stage 1, where these points join the others with the own voxel already done.  A wave none of whose
  // points lacks a bound starts at stage 1.
  const bool unbounded = in && okrange && !(b0 < __builtin_inff());
  bool own_done = false;            // stage 0 found a record in the own voxel: RES holds it, b0 is its distance
  unsigned long long res0 = 0;
  bool planned = false;
  uint32_t n_cands = 0;
  const int cx = voxel_of(px, m.inv_vs, m.trunc), cy = voxel_of(py, m.inv_vs, m.trunc), cz = voxel_of(pz, m.inv_vs, m.trunc);
  const unsigned long long kbase = pack_key(cx - 1, cy - 1, cz - 1);
  if (__ballot(unbounded) != 0ull) {  // stage 0 (wave-uniform): the own voxel of the points that have no bound
    n_cands = flat_plan_scan<OFF32>(sh, m, lane, unbounded ? (1u << 13) : 0u, kbase, px, py, pz, b0, 0x7F800000FFFFFFFFull);
    const unsigned long long r0 = sh.RES[lane];  // (n_cands > 0: somebody is unbounded)
    if (unbounded && (uint32_t)r0 != 0xFFFFFFFFu && sh.SLOWF[lane] == 0) {  // what it found becomes the bound of stage 1
      own_done = true;
      res0 = r0;
      b0 = __uint_as_float((uint32_t)(r0 >> 32));
    }
    wave_sync_lds_nn();  // (stage 1 rewrites P, RES, SLOWF and the lists)
  }
  uint32_t cmask = 0;
  planned = in && okrange && b0 < __builtin_inff();
  if (__ballot(planned) != 0ull) {  // wave-uniform
    const Gaps gx = axis_gaps(px, cx, m.vs, m.trunc), gy = axis_gaps(py, cy, m.vs, m.trunc), gz = axis_gaps(pz, cz, m.vs, m.trunc);
    cmask = 1u << 13;
    // Seven tests instead of twenty-six when, for every planned lane of the wave, the FAR face of each axis is out of reach
    // (the usual case once the bound is below a quarter voxel): a code that contains a far side has a lower bound >= that
    // face's (non-negative terms, monotone rounding), so only the codes built from the near sides can pass -- the same mask.
    const float fx = fmaxf(gx.s[0], gx.s[2]), fy = fmaxf(gy.s[0], gy.s[2]), fz = fmaxf(gz.s[0], gz.s[2]);
    const bool far_dead = (fx * 0.9999f > b0) && (fy * 0.9999f > b0) && (fz * 0.9999f > b0);
    if (__ballot(planned && !far_dead) == 0ull) {  // wave-uniform
      const bool xl = gx.s[0] <= gx.s[2], yl = gy.s[0] <= gy.s[2], zl = gz.s[0] <= gz.s[2];
      const float nx = xl ? gx.s[0] : gx.s[2], ny = yl ? gy.s[0] : gy.s[2], nz = zl ? gz.s[0] : gz.s[2];
      const uint32_t cx_ = xl ? 4u : 22u, cy_ = yl ? 10u : 16u, cz_ = zl ? 12u : 14u;  // 13 -/+ 9, 3, 1
      const uint32_t dx_ = cx_ - 13u, dy_ = cy_ - 13u;                               // (mod 2^32)
      const float lxy = nx + ny;
      cmask |= (!(nx * 0.9999f > b0)) ? (1u << cx_) : 0u;
      cmask |= (!(ny * 0.9999f > b0)) ? (1u << cy_) : 0u;
      cmask |= (!(nz * 0.9999f > b0)) ? (1u << cz_) : 0u;
      cmask |= (!(lxy * 0.9999f > b0)) ? (1u << (cy_ + dx_)) : 0u;
      cmask |= (!((nx + nz) * 0.9999f > b0)) ? (1u << (cz_ + dx_)) : 0u;
      cmask |= (!((ny + nz) * 0.9999f > b0)) ? (1u << (cz_ + dy_)) : 0u;
      cmask |= (!((lxy + nz) * 0.9999f > b0)) ? (1u << (cz_ + dx_ + dy_)) : 0u;
    } else {
#pragma unroll
      for (int c = 0; c < 27; c++) {
        if (c == 13) continue;
        const int ix = c / 9, iy = (c / 3) % 3, iz = c % 3;
        const float sx = ix == 1 ? 0.f : gx.s[ix], sy = iy == 1 ? 0.f : gy.s[iy], sz = iz == 1 ? 0.f : gz.s[iz];
        const float lb = ((sx + sy) + sz) * 0.9999f;  // quad_bounds' expression
        cmask |= (!(lb > b0)) ? (1u << c) : 0u;
      }
    }
    if (!planned) cmask = 0;
    if (own_done) cmask &= ~(1u << 13);  // (scanned in stage 0)
    if (__builtin_popcount(cmask) > kFlatMaxCand) {  // a loose bound near a voxel corner: the quad search, with the bound
      planned = false;
      cmask = 0;
    }
  }
  n_cands = flat_plan_scan<OFF32>(sh, m, lane, cmask, kbase, px, py, pz, b0,
                                  own_done ? res0 : (((unsigned long long)__float_as_uint(b0) << 32) | 0xFFFFFFFFull));
  // ---- C: the pairing ----------------------------------------------------------------------------------------------------
  bool slow = in && !planned;
  float b0s = b0;  // the bound phase D starts from
  {
    // (a wave whose stage 1 had no candidate at all has written nothing to LDS in it: a point that stage 0 served keeps its result)
    unsigned long long res = own_done ? res0 : 0xFFFFFFFFFFFFFFFFull;
    bool spilled = false;
    if (n_cands) {
      res = sh.RES[lane];
      spilled = sh.SLOWF[lane] != 0;
    }
    const uint32_t idx = (uint32_t)res;
    if (planned && !spilled && idx != 0xFFFFFFFFu) {
      const f32x4 w = *gat<OFF32>(pts4, idx);
      const float d2 = __uint_as_float((uint32_t)(res >> 32));
      const float n2 = (px * px + py * py) + pz * pz;
      const bool ok = d2 < thr2 + ang2 * n2;
      *gat<OFF32>(G(reinterpret_cast<f32x4*>(pair_q)), ic) = (f32x4){w.x, w.y, w.z, flat_signed_d2(d2, ok)};
      *gat<OFF32>(G(pair_gidx), ic) = ok ? __float_as_uint(w.w) : kNoMatch;
    } else if (planned) {
      slow = true;
      if (!spilled) b0s = __builtin_inff();  // the bound was not attained inside the block: once more, without it
    }
  }
  // ---- D: what the plan does not cover, quad-wise ---------------------------------------------------------------------
  const unsigned long long sm = __ballot(slow);
  if (sm == 0ull) return;  // wave-uniform
  const uint32_t ns = (uint32_t)__builtin_popcountll(sm);
  wave_sync_lds_nn();  // (phase B's readers of P are done)
  if (slow) {
    sh.SL[lanes_below(sm)] = (unsigned char)lane;
    sh.P[lane] = (f32x4){px, py, pz, b0s};
  }
  wave_sync_lds_nn();
  const uint32_t grp = lane >> 2, sub = lane & 3u;
  for (uint32_t g = 0; g < ns; g += 16u) {
    const uint32_t k = g + grp;
    if (k < ns) {  // whole quads
      const uint32_t p = sh.SL[k];
      const f32x4 P = sh.P[p];
      const NNResult r = nn_search_quad<OFF32>(m, sub, P.x, P.y, P.z, P.w);
      if (sub == 0u) {
        const uint32_t ip = i0 + p;
        const float n2 = (P.x * P.x + P.y * P.y) + P.z * P.z;
        const bool ok = r.found && (r.d2 < thr2 + ang2 * n2);
        *gat<OFF32>(G(reinterpret_cast<f32x4*>(pair_q)), ip) = (f32x4){r.pt.x, r.pt.y, r.pt.z, flat_signed_d2(r.d2, ok)};
        *gat<OFF32>(G(pair_gidx), ip) = ok ? __float_as_uint(r.pt.w) : kNoMatch;
      }
    }
  }
}


// The same search with the points handed over in registers and the result handed back in registers -- lane = point -- for the
// small layer's one-launch loop (k_icpw, mh_loop_wave.h), where a wave keeps its points' pairings from one ICP iteration to the
// next and nothing goes through global memory.  `in`: the lane holds a point; (px, py, pz): the point under the current pose;
// b0: the squared distance to the record paired with it in the previous iteration (attained by a map record) or +inf.
// Phases A1 (masks) | stage 0 | A2 | B | C | D exactly as in match_flat_wave: the same candidate set, the same fp32 arithmetic,
// the same 64-bit key -- the lexicographic minimum of (d2, scan position) over the 27-voxel block.
#ifdef MH_DEBUG_PHASES
static __device__ unsigned long long g_flatdbg[16];  // debug build: [0] searches (waves) [1] points [2] unbounded at entry [3] slow: out of range / no bound after stage 0
                                              // [4] slow: > kFlatMaxCand candidates [5] slow: chunk space [6] slow: bound not attained [7] candidates [8] chunks (stage 1) [9] D rounds
                                              // match_kbest_wave (mh_k_match_kbest.h): [10] points [11] without a bound [12] > kFlatMaxCand candidates [13] chunk space [14] slot k - 1 empty [15] bounded scan of the lane's own, slot k - 1 empty
#define MH_FLATDBG(i, v) do { const unsigned long long b_ = __ballot(v); if (lane == 0 && b_) atomicAdd(&g_flatdbg[i], (unsigned long long)__builtin_popcountll(b_)); } while (0)
#define MH_FLATDBG_ADD(i, v) do { if (lane == 0) atomicAdd(&g_flatdbg[i], (unsigned long long)(v)); } while (0)
#else
#define MH_FLATDBG(i, v) do { } while (0)
#define MH_FLATDBG_ADD(i, v) do { } while (0)
#endif
struct FlatHit {
  f32x4 pt;    // the nearest record {x, y, z, source index}; zeros when there is none
  float d2;    // its squared distance; +inf when there is none
  bool found;
};
template <class FW>
__device__ __forceinline__ FlatHit flat_search_points(FW& sh, const MapView& m, bool in, float px, float py, float pz, float b0) {
  constexpr int kFlatMaxCand = FW::kMaxCand;
  const uint32_t lane = (uint32_t)__lane_id();
  const gpts_ptr pts4 = (gpts_ptr)m.pts;
  const float lim = 1.0e6f;
  const bool okrange = ((int)(fabsf(px * m.inv_vs) < lim) & (int)(fabsf(py * m.inv_vs) < lim) & (int)(fabsf(pz * m.inv_vs) < lim)) != 0;
  const bool unbounded = in && okrange && !(b0 < __builtin_inff());
  bool own_empty = false;  // stage 0 scanned the own voxel and found it empty: stage 1 takes the rest of the block unbounded
  MH_FLATDBG_ADD(0, 1);
  MH_FLATDBG(1, in);
  MH_FLATDBG(2, unbounded);
  bool own_done = false;
  unsigned long long res0 = 0;
  bool planned = false;
  uint32_t n_cands = 0;
  const int cx = voxel_of(px, m.inv_vs, m.trunc), cy = voxel_of(py, m.inv_vs, m.trunc), cz = voxel_of(pz, m.inv_vs, m.trunc);
  const unsigned long long kbase = pack_key(cx - 1, cy - 1, cz - 1);
  if (__ballot(unbounded) != 0ull) {  // stage 0 (wave-uniform): the own voxel of the points that have no bound
    n_cands = flat_plan_scan(sh, m, lane, unbounded ? (1u << 13) : 0u, kbase, px, py, pz, b0, 0x7F800000FFFFFFFFull);
    const unsigned long long r0 = sh.RES[lane];
    if (unbounded && (uint32_t)r0 != 0xFFFFFFFFu && sh.SLOWF[lane] == 0) {
      own_done = true;
      res0 = r0;
      b0 = __uint_as_float((uint32_t)(r0 >> 32));
    } else if (unbounded && sh.SLOWF[lane] == 0 && kFlatMaxCand >= 27) {
      // the own voxel is empty (a third of the points of a decimated layer at ICP iteration 0): the other 26 voxels of the block
      // are planned without a bound -- every lower bound passes, nothing is narrowed, every record is compared -- and what that
      // finds, or does not find, is the block's answer
      own_empty = true;
    }
    wave_sync_lds_nn();
  }
  uint32_t cmask = 0;
  planned = in && okrange && (b0 < __builtin_inff() || own_empty);
  MH_FLATDBG(3, in && !planned);
  if (__ballot(planned) != 0ull) {  // wave-uniform
    const Gaps gx = axis_gaps(px, cx, m.vs, m.trunc), gy = axis_gaps(py, cy, m.vs, m.trunc), gz = axis_gaps(pz, cz, m.vs, m.trunc);
    cmask = 1u << 13;
    const float fx = fmaxf(gx.s[0], gx.s[2]), fy = fmaxf(gy.s[0], gy.s[2]), fz = fmaxf(gz.s[0], gz.s[2]);
    const bool far_dead = (fx * 0.9999f > b0) && (fy * 0.9999f > b0) && (fz * 0.9999f > b0);
    if (__ballot(planned && !far_dead) == 0ull) {  // the seven near-side codes (match_flat_wave has the argument)
      const bool xl = gx.s[0] <= gx.s[2], yl = gy.s[0] <= gy.s[2], zl = gz.s[0] <= gz.s[2];
      const float nx = xl ? gx.s[0] : gx.s[2], ny = yl ? gy.s[0] : gy.s[2], nz = zl ? gz.s[0] : gz.s[2];
      const uint32_t cx_ = xl ? 4u : 22u, cy_ = yl ? 10u : 16u, cz_ = zl ? 12u : 14u;
      const uint32_t dx_ = cx_ - 13u, dy_ = cy_ - 13u;
      const float lxy = nx + ny;
      cmask |= (!(nx * 0.9999f > b0)) ? (1u << cx_) : 0u;
      cmask |= (!(ny * 0.9999f > b0)) ? (1u << cy_) : 0u;
      cmask |= (!(nz * 0.9999f > b0)) ? (1u << cz_) : 0u;
      cmask |= (!(lxy * 0.9999f > b0)) ? (1u << (cy_ + dx_)) : 0u;
      cmask |= (!((nx + nz) * 0.9999f > b0)) ? (1u << (cz_ + dx_)) : 0u;
      cmask |= (!((ny + nz) * 0.9999f > b0)) ? (1u << (cz_ + dy_)) : 0u;
      cmask |= (!((lxy + nz) * 0.9999f > b0)) ? (1u << (cz_ + dx_ + dy_)) : 0u;
    } else {
#pragma unroll
      for (int c = 0; c < 27; c++) {
        if (c == 13) continue;
        const int ix = c / 9, iy = (c / 3) % 3, iz = c % 3;
        const float sx = ix == 1 ? 0.f : gx.s[ix], sy = iy == 1 ? 0.f : gy.s[iy], sz = iz == 1 ? 0.f : gz.s[iz];
        const float lb = ((sx + sy) + sz) * 0.9999f;
        cmask |= (!(lb > b0)) ? (1u << c) : 0u;
      }
    }
    if (!planned) cmask = 0;
    if (own_done || own_empty) cmask &= ~(1u << 13);
    MH_FLATDBG(4, __builtin_popcount(cmask) > kFlatMaxCand);
    if (__builtin_popcount(cmask) > kFlatMaxCand) {
      planned = false;
      cmask = 0;
    }
  }
  n_cands = flat_plan_scan(sh, m, lane, cmask, kbase, px, py, pz, b0,
                           own_done ? res0 : (((unsigned long long)__float_as_uint(b0) << 32) | 0xFFFFFFFFull));
  MH_FLATDBG_ADD(7, n_cands);
  FlatHit h;
  h.pt = (f32x4)(0.f);
  h.d2 = __builtin_inff();
  h.found = false;
  bool slow = in && !planned;
  float b0s = b0;
  {
    unsigned long long res = own_done ? res0 : 0xFFFFFFFFFFFFFFFFull;
    bool spilled = false;
    if (n_cands) {
      res = sh.RES[lane];
      spilled = sh.SLOWF[lane] != 0;
    }
    const uint32_t idx = (uint32_t)res;
    bool again = false;
    if (planned && !spilled && idx != 0xFFFFFFFFu) {
      h.pt = pts4[idx];
      h.d2 = __uint_as_float((uint32_t)(res >> 32));
      h.found = true;
    } else if (planned && !(own_empty && !spilled)) {  // (own_empty: the whole block was compared -- there is no record in it)
      slow = true;
      again = true;
      if (!spilled) b0s = __builtin_inff();
    }
    MH_FLATDBG(5, again && spilled);
    MH_FLATDBG(6, again && !spilled);
  }
  const unsigned long long sm = __ballot(slow);
  if (sm == 0ull) return h;  // wave-uniform
  const uint32_t ns = (uint32_t)__builtin_popcountll(sm);
  MH_FLATDBG_ADD(9, (ns + 15u) / 16u);
  wave_sync_lds_nn();
  if (slow) {
    sh.SL[lanes_below(sm)] = (unsigned char)lane;
    sh.P[lane] = (f32x4){px, py, pz, b0s};
  }
  wave_sync_lds_nn();
  const uint32_t grp = lane >> 2, sub = lane & 3u;
  for (uint32_t g = 0; g < ns; g += 16u) {
    const uint32_t k = g + grp;
    if (k < ns) {  // whole quads
      const uint32_t p = sh.SL[k];
      const f32x4 P = sh.P[p];
      const NNResult r = nn_search_quad(m, sub, P.x, P.y, P.z, P.w);
      if (sub == 0u) {  // handed back to the point's lane: the record in P, (d2 | found) in RES
        sh.P[p] = r.pt;
        sh.RES[p] = ((unsigned long long)__float_as_uint(r.d2) << 32) | (r.found ? 1ull : 0ull);
      }
    }
  }
  wave_sync_lds_nn();
  if (slow) {
    const unsigned long long rr = sh.RES[lane];
    h.pt = sh.P[lane];
    h.d2 = __uint_as_float((uint32_t)(rr >> 32));
    h.found = (rr & 1ull) != 0ull;
  }
  wave_sync_lds_nn();  // (the next search rewrites P and RES)
  return h;
}

}  // namespace mh
