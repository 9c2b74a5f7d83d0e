// COMPRESSING on the device: snappy raw compress / uncompress, byte-identical to
// snappy 1.1.8 (the version the reference links; compressing.h:8-37 ->
// SArray::CompressTo / UncompressFrom, shared_array_inl.h:232-255).
//
// Compress.  A snappy stream is varint32(n) followed by the greedy LZ77 parse
// of each 64 KiB input fragment, and every fragment is parsed on its own (fresh
// hash table, no references across fragments).  A wave runs the exact 1.1.8
// parse of a fragment with lane-parallel helpers -- 64 speculative probes of
// the skip heuristic per step (the probe positions do not depend on the data,
// only on where the skip loop started), match extension 64 bytes per step,
// literal bytes copied 64 per step.  Fragments with no match at all (one
// literal: incompressible data) are found first by a probe-only pass that
// reads the input where the skip loop probes; the others are parsed in LDS.
// Fragment offsets come from a per-stream scan of the fragment lengths, and a
// last launch places tags and literals (snappy_parse / _scan / _place;
// no workgroup waits for another).
//
// Uncompress accepts any valid snappy stream (a reference sender's included)
// and reproduces RawUncompress's verdict.  First every output fragment is
// assumed stored as one literal where a 1.1.8 encoder of incompressible data
// puts it, checked and copied (K-spec; such a stream is done there).
// Otherwise tag boundaries are found in parallel: a one-wave linker hops over
// stored fragments (K0); if it meets too many small tags, every 4 KiB window
// of the compressed bytes is parsed speculatively from each of its first 64
// offsets (K1) and one lane links the windows (K2) -- the true chain enters a
// window on one of those chains almost always, and their bookkeeping gives the
// exit and the output count.  K3 re-walks each window from its true entry,
// validates every copy (1 <= offset <= produced) and indexes the tag that
// starts each 64 KiB output fragment.  K4 decodes the output fragments in
// parallel in LDS.  A stream whose tags straddle output fragments or whose
// copies reach into an earlier fragment (never produced by a 1.1.8 encoder,
// but valid) is decoded by one lane instead (K5).
//
// This file is the launch layer -- scratch sizes, the job tables, the launches
// -- and the one translation unit of COMPRESSING.  The kernels are in
// snappy_compress.h and snappy_uncompress.h (in that order: the object's
// kernel order), what both use in snappy_common.h.
#include "psf_internal.h"

#include <algorithm>
#include <atomic>
#include "ff_dequant.h"
#include "snappy_common.h"
#include "snappy_compress.h"
#include "snappy_uncompress.h"

namespace psf {

size_t snappy_max_compressed(size_t n) { return 32 + n + n / 6; }

namespace {
// The compressor's scratch, as byte offsets: tag slots (at 0) | finfo | offset
// (one each per fragment) | in_place (per job) | stash (per fragment), and
// 64 bytes to spare.
struct CScratch {
  size_t finfo, offset, in_place, stash, bytes;
  explicit CScratch(size_t nfrag) {
    finfo = nfrag * kSnappyFragOut;
    offset = finfo + nfrag * 8;
    in_place = offset + nfrag * 8;
    stash = in_place + 4 * kSnappyBatchMax;
    bytes = stash + nfrag * kStash + 64;
  }
};
}  // namespace

size_t snappy_compress_batch_scratch(const SnappyCJob* jobs, int njobs) {
  size_t nfrag = 0;
  for (int i = 0; i < njobs; ++i) nfrag += (jobs[i].n + kFrag - 1) / kFrag;
  return CScratch(nfrag).bytes;
}

size_t snappy_compress_scratch(size_t n) {
  const SnappyCJob j{nullptr, n, nullptr, 0, 0};
  return snappy_compress_batch_scratch(&j, 1);
}

int snappy_compress_batch_launch(const SnappyCJob* jobs, int njobs, void* scratch, hipStream_t st, Profiler* prof,
                                 PubSlot* pub_base) {
  if (njobs <= 0 || njobs > kSnappyBatchMax) return kErrArg;
  SnappyCJobs K{};
  K.pub = pub_base;
  K.njobs = (uint32_t)njobs;
  double bytes = 0;
  for (int i = 0; i < njobs; ++i) {
    const SnappyCJob& q = jobs[i];
    if (q.n == 0 || q.n > 0xffffffffull) return kErrArg;
    CJob& c = K.j[i];
    c.in = static_cast<const uint8_t*>(q.in);
    c.dst = static_cast<uint8_t*>(q.out);
    c.n = q.n;
    c.frag0 = K.nfrag;
    c.nfrag = (uint32_t)((q.n + kFrag - 1) / kFrag);
    c.hdr = 1;
    for (uint64_t v = q.n; v >= 128; v >>= 7) ++c.hdr;
    c.slot = (uint32_t)q.slot;
    c.ticket = q.ticket;
    c.stored = q.stored ? 1u : 0u;
    K.nfrag += c.nfrag;
    bytes += (double)q.n;
  }
  uint8_t* s = static_cast<uint8_t*>(scratch);
  const CScratch L(K.nfrag);  // (every word the kernels read is written first in the chain)
  K.finfo = reinterpret_cast<uint64_t*>(s + L.finfo);
  K.offset = reinterpret_cast<uint64_t*>(s + L.offset);
  K.in_place = reinterpret_cast<uint32_t*>(s + L.in_place);
  K.stash = s + L.stash;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return kErrHip;
  // K-parse: persistent workgroups, one per CU (the parse's LDS footprint allows no more)
  const uint32_t grid = K.nfrag < (uint32_t)cus ? K.nfrag : (uint32_t)cus;
  ProfScope ps(prof, kKSnappyCompress, st, bytes);
  uint32_t longest = 0;
  for (int i = 0; i < njobs; ++i) longest = std::max(longest, K.j[i].nfrag);
  if (longest <= kInlineScan) K.offset = nullptr;  // K-place sums the lengths itself
  hipLaunchKernelGGL(snappy_parse, dim3(grid), dim3(kCThreads), 0, st, K, s);
  if (K.offset) hipLaunchKernelGGL(snappy_scan, dim3(K.njobs), dim3(kScanT), 0, st, K);
  hipLaunchKernelGGL(snappy_place, dim3(K.nfrag), dim3(kPlaceT), 0, st, K, s);
  return launch_status();
}

int snappy_compress_launch(const void* in, size_t n, void* out, void* scratch, hipStream_t st, Profiler* prof,
                           PubSlot* pub, uint32_t ticket) {
  const SnappyCJob j{in, n, out, 0, ticket};
  return snappy_compress_batch_launch(&j, 1, scratch, st, prof, pub);
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the batch's control words (SnappyDJobs::ctrl): 8 per stream, then one spare
// word; the streams' index arrays start at the next multiple of 256
static size_t ctrl_bytes(int njobs) { return (size_t)njobs * 32 + 4; }
static size_t ctrl_region(int njobs) { return align256(ctrl_bytes(njobs)); }

// one stream's index arrays (DScr, LinkBlk): the bytes allocated for them
static size_t djob_bytes(size_t C, size_t dsize) {
  const size_t nwin = (C + kWin - 1) / kWin + 1;
  const size_t nfo = (dsize + kFrag - 1) / kFrag + 1;
  const size_t nblk = (nwin + kLinkPer - 1) / kLinkPer + 1;  // linker blocks (LinkBlk)
  return align256(nwin * (kWin / 8) + C * 4 + nwin * 8 * (2 * kStarts + 2) + 4 * nfo * 8 + 64 +
                  nblk * (kStarts * 9 + 12) + 16);
}

// a stream's windows and output fragments, as the kernels count them
static void djob_shape(DJob& D, size_t C, uint32_t hdr, size_t dsize) {
  D.C = C;
  D.dsize = dsize;
  D.hdr = hdr;
  D.nwin = (uint32_t)((C - hdr + kWin - 1) / kWin);
  D.nfo = (uint32_t)((dsize + kFrag - 1) / kFrag);
}

// Where those arrays end as the kernels carve them (dscr, link_blk), in bytes
// from the stream's scratch: must not exceed djob_bytes (tests/test_snappy_layout.py).
static size_t djob_layout_end(size_t C, uint32_t hdr, size_t dsize) {
  SnappyDJobs K{};
  DJob& D = K.j[0];  // (scratch null: the pointers are offsets)
  djob_shape(D, C, hdr, dsize);
  const LinkBlk B = link_blk(D, dscr(K, D, 0));
  return reinterpret_cast<uintptr_t>(B.F + (size_t)(link_nblk(D.nwin) + 1) * kStarts);
}

size_t snappy_uncompress_batch_scratch(const SnappyDJob* jobs, int njobs) {
  size_t b = ctrl_region(njobs);
  for (int i = 0; i < njobs; ++i) b += djob_bytes(jobs[i].c, jobs[i].dsize);
  return b;
}

bool snappy_dequant_ok(const SnappyDequant& dq, size_t dsize) {
  return dq.values && (dq.nb == 1 || dq.nb == 2) && (dq.value_type == kFloat || dq.value_type == kDouble) &&
         dsize > 0 && dsize % (size_t)dq.nb == 0 && (reinterpret_cast<uintptr_t>(dq.values) & 15) == 0;
}

size_t snappy_uncompress_scratch(size_t C, size_t dsize) { return ctrl_region(1) + djob_bytes(C, dsize); }

// K1-K3 and K4 (+ K5) of a batch whose fast path has run.  K2a / K2c / K3
// loop over their blocks / windows on grids capped at about twice what the
// chip holds at once (K3: 32 waves per CU), so a stream they have nothing to
// do for (stored fragments: K-spec decoded it) costs a few thousand
// workgroups, not one per 4 KiB window.  K1 keeps one workgroup per window:
// with a capped grid each workgroup's share of windows is fixed and the
// tag-dense scan lost its dynamic balance (sorted keys, 128 MiB: K1 0.83 ->
// 0.95 ms at twice its residency, 1.04 at once; measured with an A/B script
// that is not kept in the tree).  K2a-c link the streams whose chain enters
// every window at one of its first 64 bytes; K2 walks what they leave.
constexpr uint32_t kIndexGrid = 16384, kLinkGrid = 1024;
static int launch_tail(const SnappyDJobs& K, hipStream_t st) {
  if (K.nwin) {
    hipLaunchKernelGGL(snappy_dscan, dim3(K.nwin), dim3(64), 0, st, K);
    hipLaunchKernelGGL(snappy_dlinka, dim3(min(K.nblk, kLinkGrid)), dim3(64), 0, st, K);
    hipLaunchKernelGGL(snappy_dlinkb, dim3(K.njobs), dim3(kLinkWaves * 64), 0, st, K);
    hipLaunchKernelGGL(snappy_dlinkc, dim3(min(K.nblk, kLinkGrid)), dim3(64), 0, st, K);
    hipLaunchKernelGGL(snappy_dlink, dim3(K.njobs), dim3(64), 0, st, K);
    hipLaunchKernelGGL(snappy_dindex, dim3(min(K.nwin, kIndexGrid)), dim3(64), 0, st, K);
  }
  hipLaunchKernelGGL(snappy_dfrag, dim3(K.nfo1), dim3(256), 0, st, K);
  return launch_status();
}

// Launches for the whole batch: K-spec (+ K0 in one more workgroup per
// stream), then the tail: K1, K2a-c, K2, K3 (one launch each), K4 (+ K5 in
// each stream's last workgroup).  On streams of stored fragments K-spec
// decodes everything and the others return at once.
int snappy_uncompress_batch_launch(const SnappyDJob* jobs, int njobs, void* scratch, hipStream_t st,
                                   Profiler* prof, PubSlot* pub_base, const ZeroPair& z, SnappyTail* tail) {
  if (njobs <= 0 || njobs > kSnappyBatchMax) return kErrArg;
  SnappyDJobs K{};
  uint8_t* s = static_cast<uint8_t*>(scratch);
  K.ctrl = reinterpret_cast<uint32_t*>(s);  // (ctrl_bytes)
  K.pub = pub_base;
  K.njobs = (uint32_t)njobs;
  uint8_t* data = s + ctrl_region(njobs);
  double bytes = 0;
  for (int i = 0; i < njobs; ++i) {
    const SnappyDJob& q = jobs[i];
    if (q.hdr == 0 || q.hdr > q.c || q.hdr > 5) return kErrArg;
    DJob& D = K.j[i];
    D.in = static_cast<const uint8_t*>(q.in);
    D.out = static_cast<uint8_t*>(q.out);
    D.scratch = data;
    djob_shape(D, q.c, q.hdr, q.dsize);
    D.fo0 = K.nfo1;
    D.win0 = K.nwin;
    D.blk0 = K.nblk;
    D.slot = (uint32_t)q.slot;
    D.ticket = q.ticket;
    if (q.dq.values) {
      if (!snappy_dequant_ok(q.dq, q.dsize)) return kErrArg;
      D.fv = q.dq.values;
      D.frange = q.dq.range;
      D.fratio = ff_ratio(q.dq.nb);
      D.fmn = q.dq.mn;
      D.fmx = q.dq.mx;
      D.fnb = (uint32_t)q.dq.nb;
      D.fdbl = q.dq.value_type == kDouble ? 1u : 0u;
    }
    K.nfo1 += D.nfo ? D.nfo : 1;  // an empty output still takes one workgroup (header check, verdict)
    K.nwin += D.nwin;
    K.nblk += link_nblk(D.nwin);
    data += djob_bytes(q.c, q.dsize);
    bytes += (double)q.c +
             (q.dq.values ? (double)(q.dsize / q.dq.nb) * (q.dq.value_type == kDouble ? 8 : 4) : (double)q.dsize);
  }
  const size_t zneed = ctrl_bytes(njobs);
  if (z.cur && zneed <= z.bytes) {  // the context's region the previous launch cleared
    K.ctrl = static_cast<uint32_t*>(z.cur);
    K.znext = static_cast<uint32_t*>(z.next);
    K.zwords = (uint32_t)(z.bytes / 4);
  } else if (hipMemsetAsync(K.ctrl, 0, zneed, st) != hipSuccess) {
    return kErrHip;
  }
  std::shared_ptr<SnappyDJobs> keep;
  if (tail) keep = std::make_shared<SnappyDJobs>(K);
  {  // the profiler brackets K-spec alone when the tail is deferred, else K-spec and the tail
    ProfScope ps(prof, kKSnappyDecompress, st, bytes);
    hipLaunchKernelGGL(snappy_dspec, dim3(K.nfo1 + K.njobs), dim3(256), 0, st, K);
    if (!tail) return launch_tail(K, st);
  }
  tail->jobs = keep;
  tail->pending = true;
  return launch_status();
}

// (not bracketed by the profiler: the batch's bytes were counted with its fast
// path, whose launch the bench times)
int snappy_uncompress_tail_launch(SnappyTail* tail, hipStream_t st) {
  if (!tail || !tail->pending || !tail->jobs) return kErrArg;
  tail->pending = false;
  const SnappyDJobs& K = *static_cast<const SnappyDJobs*>(tail->jobs.get());
  return launch_tail(K, st);
}

int snappy_uncompress_launch(const void* in, size_t C, uint32_t hdr, size_t dsize, void* out, void* scratch,
                             hipStream_t st, Profiler* prof, PubSlot* pub, uint32_t ticket) {
  const SnappyDJob j{in, C, hdr, dsize, out, 0, ticket};
  return snappy_uncompress_batch_launch(&j, 1, scratch, st, prof, pub, ZeroPair{});
}

}  // namespace psf

// tests (tests/test_snappy_layout.py): for one stream of C compressed bytes
// (hdr of them the varint header) and dsize output bytes, where the kernels'
// index arrays end and how many bytes the scratch size allows them.  Launches
// nothing.
extern "C" int psf_debug_snappy_dscratch(size_t C, uint32_t hdr, size_t dsize, size_t* end, size_t* bytes) {
  if (hdr == 0 || hdr > C || hdr > 5 || !end || !bytes) return psf::kErrArg;
  *end = psf::djob_layout_end(C, hdr, dsize);
  *bytes = psf::djob_bytes(C, dsize);
  return psf::kOk;
}

#ifdef PSF_SNAPPY_TRACE
// diagnostic builds: copy the kernels' phase timestamps out
extern "C" int psf_debug_dfrag_trace(void* out, size_t bytes) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(psf::g_dfrag_trace), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess
             ? 0
             : -4;
}
extern "C" int psf_debug_snappy_trace(void* out, size_t bytes) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(psf::g_snappy_trace), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess
             ? 0
             : -4;
}
#endif
