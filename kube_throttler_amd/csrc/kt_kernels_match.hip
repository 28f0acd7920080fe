// kt_kernels_match.hip — kt_build_match_cache: the match cache of single-chunk programs (kt_scan.h: replay_tile), gfx950.
#include "kt_scan.h"

namespace kt {

// ---------------------------------------------------------------------------------------------------
// kt_build_match_cache — mw[k][row] = what scan_tile hands to post() for entry rng.x + k of the namespace list of pod `row`:
// the terms of that word the pod matches (exact: cached programs have no `slow` shapes).  Zero where the list is shorter and
// for rows without a valid pod.  The chunk is staged as the ONE forms of the scans stage it, a wave owns a tile of 64 rows,
// lane = row, and runs the very scan_tile of those forms with a post hook that stores the word and keeps nothing for the peel:
// every lane that still has words advances in every round, so the (wave-uniform) round counter IS the lane's list position.
//   rows == nullptr : rows [0, n)          (after a compile: one launch over every row ever fed)
//   rows != nullptr : the n listed rows    (pod events: the rows whose atom rows were rewritten; a row may be listed twice —
//                                           both lanes store the same words)
// Runs where the atom rows are written and nowhere else: nothing a reconcile or a check changes enters these words.
// Write-through (a.vx != nullptr): the countable scan view keeps the planes of its records in scan order (MatchViewPlanes,
// kt_index.h) and every word stored for a row goes to the row's record as well — the row -> record table is read once per lane,
// beside the meta word.
// Match-code records (a.mc != nullptr; kt_match_codes.h): the lane also applies the sweep's run rule to every word it stores — the
// run masks of the chunk's words are staged from the index's side table (BmIndexArgs-independent: a.runs) beside the image —
// appends the codes of what is left to a record in registers and stores the record once behind the scan.  A row without a
// valid pod gets count 0, a row listed twice stores the same record twice.  Only for tables of at most kMatchReplay planes.
// ---------------------------------------------------------------------------------------------------
struct MatchBuildArgs {
  const uint64_t* meta;
  const uint16_t* latom;
  const int64_t* rows;
  uint64_t* mw;
  uint64_t stride;   // words per plane
  uint32_t planes;   // planes to write (<= kMatchPlanes)
  uint32_t n;        // rows [0, n) or list entries
  uint32_t cap;      // rows a plane holds: a listed row at or beyond it is skipped
  uint64_t* vx;      // nullable: the view's planes ...
  const int32_t* vpos;  // ... its row -> record table (-1: no record) ...
  uint64_t vstride;  // ... and its words per plane: a record at or beyond it is skipped
  MatchCodes* vmc;       // nullable: the view's match-code records (write-through beside vx)
  MatchCodes* mc;        // nullable: the match-code record of every pod row ...
  const uint64_t* runs;  // ... and the {seg_lo, seg_hi} of the chunk's words they are cut with (nullable: no throttle has several terms)
  uint32_t off_runs;     // ... in LDS
  BmIndexArgs ix;
  BmChunk ch;
};

template <bool VETO, int NEED>
__global__ __launch_bounds__(kBlockIx) void kt_build_match_cache(const MatchBuildArgs a) {
  constexpr int LA = 8;
  KT_LDS unsigned char* lds = (KT_LDS unsigned char*)kt_smem;
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const BmChunk& ch = a.ch;
  {
    const StageSeg segs[2] = {chunk_image_segment(a.ix, ch), StageSeg{a.off_runs, (const u32x4*)a.runs, a.runs ? ch.n_words : 0u}};
    lds_stage_segments<2, 4>(lds, segs);
  }
  const bool codes = a.mc != nullptr, seg_on = a.runs != nullptr;  // wave-uniform
  KT_LDS const u64x2* runs = (KT_LDS const u64x2*)(lds + a.off_runs);
  const BmView bm = open_chunk<VETO>(lds, a.ix, ch);
  __syncthreads();
  const uint32_t n = a.n, planes = a.planes;
  const uint32_t n_wtiles = (n + kWave - 1u) / kWave;
  const uint32_t wstep = gridDim.x * (uint32_t)(kBlockIx / kWave);
  for (uint32_t wt = blockIdx.x * (uint32_t)(kBlockIx / kWave) + wave; wt < n_wtiles; wt += wstep) {
    // always from valid addresses: lanes past the end re-read the last entry and store nothing
    const uint32_t i = wt * kWave + lane;
    const uint32_t ic = min(i, n - 1u);
    const uint32_t p = a.rows ? (uint32_t)a.rows[ic] : ic;
    const bool in = i < n && p < a.cap;
    const uint32_t pc = min(p, a.cap - 1u);
    const uint64_t meta = a.meta[pc];
    const int32_t vj = a.vx ? a.vpos[pc] : -1;
    u32x4 raw[1];
    load_atoms<LA>(a.latom, (int64_t)pc, raw);
    const bool on = in && ((meta >> kMetaStateShift) & kPodValid) != 0;
    const uint32_t ns = on ? (uint32_t)(meta & kMetaNsMask) : 0u;
    uint32_t ro[LA];
    atom_row_offsets<LA>(raw, ro);
    uint64_t* q = a.mw + pc;
    const bool thru = in && vj >= 0 && (uint64_t)vj < a.vstride;  // (false everywhere without a view: vj = -1)
    uint64_t* qv = a.vx + (thru ? (uint32_t)vj : 0u);
    uint32_t round = 0u;  // wave-uniform
    MatchCodes rec{0ull, 0ull};
    scan_tile<LA, VETO, NEED, false>(
        bm, on, ns, ro, [&](bool, uint32_t) {}, [&](uint32_t) { return true; },
        [&](uint32_t w, uint64_t xx, int) -> uint64_t {
          if (in && round < planes) q[(uint64_t)round * a.stride] = xx;
          if (thru && round < planes) qv[(uint64_t)round * a.vstride] = xx;
          if (codes && round < kMatchCodeLists) {  // (a lane that did not advance has xx = 0; its w is stale but in range)
            uint64_t x = xx;
            if (seg_on) {
              const u64x2 seg = runs[w];
              x = match_run_rule(x, seg.x, seg.y);
            }
            while (x) {  // lane-divergent: a handful of bits
              const uint32_t bit = (uint32_t)__ffsll((unsigned long long)x) - 1u;
              x &= x - 1ull;
              match_codes_append(rec, match_code(round, bit));
            }
          }
          round += 1u;
          return 0ull;
        });
    if (codes && in) a.mc[pc] = rec;
    if (codes && thru && a.vmc) a.vmc[(uint32_t)vj] = rec;
    for (; round < planes; ++round) {  // the planes past the longest list of the tile
      if (in) q[(uint64_t)round * a.stride] = 0ull;
      if (thru) qv[(uint64_t)round * a.vstride] = 0ull;
    }
  }
}

// kt_gather_match_planes — the planes of a freshly built countable view: mx[k][j] = mw[k][rows[j]], thread = record
// (codes / vmc, nullable: and the row's match-code record, vmc[j] = codes[rows[j]])
__global__ __launch_bounds__(256) void kt_gather_match_planes(const uint64_t* mw, uint64_t stride, uint32_t planes, const int64_t* rows, int64_t n,
                                                             uint64_t* mx, uint64_t mx_stride, const MatchCodes* codes, MatchCodes* vmc) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
    const uint64_t p = (uint64_t)rows[j];
    if (p >= stride) continue;  // (never: the list holds rows of the pod table)
    uint64_t x[kMatchReplay];
#pragma unroll
    for (int k = 0; k < kMatchReplay; ++k) x[k] = (uint32_t)k < planes ? mw[(uint64_t)k * stride + p] : 0ull;
#pragma unroll
    for (int k = 0; k < kMatchReplay; ++k)
      if ((uint32_t)k < planes) mx[(uint64_t)k * mx_stride + (uint64_t)j] = x[k];
    if (vmc) vmc[j] = codes[p];
  }
}
void launch_gather_match_planes(const uint64_t* mw, uint64_t stride, uint32_t planes, const int64_t* rows, int64_t n, uint64_t* mx,
                                uint64_t mx_stride, hipStream_t s, const MatchCodes* codes, MatchCodes* vmc) {
  if (n <= 0 || !mw || !mx || planes == 0u || planes > (uint32_t)kMatchReplay || (uint64_t)n > mx_stride) return;
  const int64_t nb = std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(kt_gather_match_planes, dim3((unsigned)nb), dim3(256), 0, s, mw, stride, planes, rows, n, mx, mx_stride, codes,
                     codes ? vmc : nullptr);
}

bool match_cache_fits(const IndexDev& ix) {
  if (ix.n_chunks != 1 || ix.h_chunks.size() != 1 || ix.n_slow != 0 || ix.has_long || ix.la > 8u || ix.max_need > 3u) return false;
  const BmChunk& ch = ix.h_chunks[0];
  return !ch.has_slow && ch.n_words != 0u && ix.bm_max_lds <= (uint32_t)kMaxLds;
}

bool match_codes_fit(const IndexDev& ix, uint32_t planes) {
  if (!match_cache_fits(ix) || planes == 0u || planes > (uint32_t)kMatchReplay) return false;
  const BmChunk& ch = ix.h_chunks[0];
  if (!ch.has_adj) return true;
  // the image (16-byte granules) and the run masks of the chunk's words behind it
  return ix.bm_runs != nullptr && ((ix.bm_max_lds + 15u) & ~15u) + ch.n_words * 16u <= (uint32_t)kMaxLds;
}

bool launch_build_match_cache(const PodTable& pods, int64_t n, const int64_t* rows_dev, const IndexDev& ix, uint64_t* mw, uint64_t stride,
                              uint32_t planes, hipStream_t s, const MatchViewPlanes* view, MatchCodes* codes) {
  if (n <= 0) return true;
  if (!match_cache_fits(ix) || pods.LA > 8 || !mw || planes == 0u || planes > (uint32_t)kMatchPlanes || stride == 0u || n > (int64_t)stride)
    return false;
  MatchBuildArgs a{};
  a.meta = pods.meta, a.latom = pods.latom, a.rows = rows_dev, a.mw = mw, a.stride = stride, a.planes = planes;
  a.n = (uint32_t)n, a.cap = (uint32_t)std::min<uint64_t>(stride, 0x80000000ull);
  if (view && view->mx && view->pos && view->stride) a.vx = view->mx, a.vpos = view->pos, a.vstride = view->stride, a.vmc = view->mc;
  uint32_t o = 0;
  auto take = [&](uint32_t bytes) { uint32_t r = o; o += (bytes + 15u) & ~15u; return r; };
  plan_bitmap_index(ix, a.ix, take);
  a.ch = ix.h_chunks[0];
  // (records only where match_codes_fit says so — the engine asks the same question before it hands the buffer over; a program
  //  whose run masks do not fit beside its image keeps its planes and gets no records)
  if (codes && match_codes_fit(ix, planes)) {
    a.mc = codes;
    if (a.ch.has_adj) a.runs = ix.bm_runs + (size_t)a.ch.w0 * 2, a.off_runs = take(a.ch.n_words * 16u);
  } else {
    a.vmc = nullptr;
  }
  const uint32_t lds_bytes = o;
  const int64_t tiles = (n + kWave - 1) / kWave, per_wg = kBlockIx / kWave;
  const int64_t nb = std::min<int64_t>((tiles + per_wg - 1) / per_wg, 2 * kCUs);
  dim3 g_((unsigned)nb), b_(kBlockIx);
#define KT_MATCH_LAUNCH(VETO_, NEED_)                                                                           \
  {                                                                                                             \
    auto kfn = kt_build_match_cache<VETO_, NEED_>;                                                              \
    (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);    \
    hipLaunchKernelGGL(kfn, g_, b_, lds_bytes, s, a);                                                           \
  }
#ifdef KT_FAST_BUILD
  KT_MATCH_LAUNCH(false, 2)
#else
  if (!ix.rich) KT_MATCH_LAUNCH(false, 2) else KT_MATCH_LAUNCH(true, 3)
#endif
#undef KT_MATCH_LAUNCH
  return true;
}

}  // namespace kt
