// Ingest kernel of lmx_ctx_upload_device: frames that already live in device memory go into a frame set's level-0 buffers, through the
// node-side steps of lmx_ctx_upload_raw or as a plain pitched copy.  The work item, the two paths and their selection rule are
// lmx_ingest.hpp; this file is the parallel shape:
//
//   k_ingest<MODE>   grid (ceil(items per frame / 256), frames), 256 lanes; lane t of workgroup b takes item 256 b + t of frame blockIdx.y:
//                    one 16-byte chunk of the result row on kRows consecutive rows.  Consecutive lanes take consecutive chunks, so a
//                    wave loads and stores runs of 1 KiB (3 KiB with the MONO8 -> BGR expansion).  The frame's {pointer, row stride} comes
//                    from a table (one entry per frame), so every frame may have its own pitch and alignment and hence its own path.
//                    No LDS, no barrier: what neighbouring outputs share is shared in registers along the strip.
// One launch per modality (launch_ingest), timed under K_PRE by the caller.
#include "lmx_internal.hpp"
#include "lmx_ingest.hpp"

namespace lmx {
namespace {

static_assert(sizeof(PullEntry) == sizeof(ingest::Entry) && offsetof(PullEntry, row_stride) == offsetof(ingest::Entry, row_stride), "the table is the frame set's PullEntry table");

template <int MODE>
__global__ __launch_bounds__(ingest::kBlock) void k_ingest(ingest::Args a, const ingest::Entry* __restrict__ tab) {
  const uint32_t item = blockIdx.x * ingest::kBlock + threadIdx.x;
  if (item >= ingest::items_per_frame(a)) return;
  ingest::run_item<MODE>(a, tab[blockIdx.y], blockIdx.y, item);
}

}  // namespace

void launch_ingest(hipStream_t s, int mode, const ingest::Args& a, const PullEntry* tab /* device-visible */, int n_frames) {
  const dim3 grid((ingest::items_per_frame(a) + ingest::kBlock - 1) / ingest::kBlock, (unsigned)n_frames);
  const ingest::Entry* t = reinterpret_cast<const ingest::Entry*>(tab);
  switch (mode) {
    case ingest::COPY: hipLaunchKernelGGL(k_ingest<ingest::COPY>, grid, dim3(ingest::kBlock), 0, s, a, t); break;
    case ingest::BLUR1: hipLaunchKernelGGL(k_ingest<ingest::BLUR1>, grid, dim3(ingest::kBlock), 0, s, a, t); break;
    case ingest::BLUR3: hipLaunchKernelGGL(k_ingest<ingest::BLUR3>, grid, dim3(ingest::kBlock), 0, s, a, t); break;
    default: hipLaunchKernelGGL(k_ingest<ingest::FLOAT_MM>, grid, dim3(ingest::kBlock), 0, s, a, t); break;
  }
}

}  // namespace lmx
