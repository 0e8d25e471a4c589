// Batch cut of a device-resident ragged u8 dataset (TRAIN --resident): ifcbk_roi_gather.  From n dataset indices it builds the compact
// batch an upload of neuston_data.collate_rois' output would have put on the device: heights, widths, the exclusive prefix sum of
// h * w * in_channels (n + 1 entries, the last one the total) and the ROIs' bytes back to back.
//
// Two kernels, both stream-ordered, no host sync, no workspace:
//   roi_gather_scan_kernel   ONE block of GS threads, IFCBK_ROI_GATHER_MAX_N / GS entries per thread: gathers hs / ws through idx and scans
//                            the byte counts (64-bit; wave scan by shuffles, the 16 wave totals through LDS)
//   roi_gather_copy_kernel   the ragged copy.  Its grid is cut from dst_capacity alone -- never from device data -- in chunks of
//                            IFCBK_ROI_GATHER_CHUNK destination bytes; a chunk at or past dst_offs[n] exits.  A ROI is anything from one
//                            byte to over a megabyte, so the work is cut by DESTINATION bytes and each piece finds its ROI by binary
//                            search in dst_offs (n + 1 <= 4097 entries, the same few cache lines for every thread).
// The destination is cut into the 16-byte units of its ABSOLUTE address, one unit per thread and step.  A unit that lies inside one ROI
// is fetched as the one or two aligned 16-byte units of the SOURCE that hold its bytes (each of them holds at least one byte of the
// ROI, so neither leaves the blob's pages), shifted into place and stored as one aligned vector: source and destination alignments are
// independent.  A unit that holds a ROI boundary, or the batch's first or last bytes, moves byte by byte.  Every destination byte is
// written by exactly one thread; no byte outside [dst_pixels, dst_pixels + min(dst_offs[n], dst_capacity)) is written and src_* is
// only read, so repeated indices are plain repeated reads.
#include "common.h"

namespace {

constexpr int GS = 1024;                                   // threads of the scan block
constexpr int GITEMS = IFCBK_ROI_GATHER_MAX_N / GS;        // entries per thread
constexpr int GT = 256;                                    // threads per copy block
constexpr int GUNITS = 4;                                  // 16-byte units per thread and chunk
static_assert(GITEMS * GS == IFCBK_ROI_GATHER_MAX_N, "the scan block covers IFCBK_ROI_GATHER_MAX_N entries");
static_assert(GT * GUNITS * 16 == IFCBK_ROI_GATHER_CHUNK, "a copy block covers IFCBK_ROI_GATHER_CHUNK destination bytes");

__global__ __launch_bounds__(GS) void roi_gather_scan_kernel(const int32_t* src_hs, const int32_t* src_ws, const int64_t* idx, int n, int ch,
                                                             int64_t* dst_offs, int32_t* dst_hs, int32_t* dst_ws) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long len[GITEMS], sum = 0;
#pragma unroll
    for (int j = 0; j < GITEMS; ++j) {
        const int k = tid * GITEMS + j;
        len[j] = 0;
        if (k < n) {
            const int64_t i = idx[k];
            const int h = src_hs[i], w = src_ws[i];
            dst_hs[k] = h;
            dst_ws[k] = w;
            len[j] = (h > 0 && w > 0) ? (long long)h * w * ch : 0;       // an empty or negative entry holds no bytes
        }
        sum += len[j];
    }
    long long inc = sum;                                     // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    __shared__ long long wsum[GS / 64];
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long run = inc - sum;
    for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
    for (int j = 0; j < GITEMS; ++j) {
        const int k = tid * GITEMS + j;
        if (k < n) dst_offs[k] = run;
        run += len[j];
        if (k == n - 1) dst_offs[n] = run;
    }
}

__global__ __launch_bounds__(GT) void roi_gather_copy_kernel(const uint8_t* src, const int64_t* src_offs, const int64_t* idx, int n,
                                                             uint8_t* dst, int64_t cap, const int64_t* dst_offs) {
    int64_t total = dst_offs[n];
    if (total > cap) total = cap;
    const int64_t dhead = (int64_t)((uintptr_t)dst & 15);
    const int64_t u0 = (int64_t)blockIdx.x * (GT * GUNITS);
    if (total <= 0 || u0 * 16 - dhead >= total) return;
#pragma unroll 1
    for (int k = 0; k < GUNITS; ++k) {
        const int64_t u = u0 + k * GT + threadIdx.x;
        const int64_t b0 = u * 16 - dhead;                   // of the unit's first byte, from dst's first
        if (b0 >= total) break;
        const int64_t b = b0 < 0 ? 0 : b0;
        const int64_t e = b0 + 16 < total ? b0 + 16 : total;
        int lo = 0, hi = n;                                  // dst_offs[lo] <= b < dst_offs[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (dst_offs[mid] <= b) lo = mid; else hi = mid;
        }
        int64_t o = dst_offs[lo], nx = dst_offs[lo + 1];
        const uint8_t* sp = src + src_offs[idx[lo]];
        if (b0 >= 0 && b0 + 16 <= total && b0 + 16 <= nx) {
            const uint8_t* p = sp + (b0 - o);
            const unsigned sh = (unsigned)((uintptr_t)p & 15);
            const uint4* q = reinterpret_cast<const uint4*>(p - sh);
            const uint4 A = q[0];
            uint4 B = make_uint4(0, 0, 0, 0);
            if (sh) B = q[1];                                // holds byte 16 - sh .. of the unit: inside the ROI
            const unsigned w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
            const unsigned dq = sh >> 2, r = sh & 3;
            unsigned t[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) t[j] = dq == 0 ? w[j] : dq == 1 ? w[j + 1] : dq == 2 ? w[j + 2] : w[j + 3];
            uint4 v;
            v.x = __builtin_amdgcn_alignbyte(t[1], t[0], r);
            v.y = __builtin_amdgcn_alignbyte(t[2], t[1], r);
            v.z = __builtin_amdgcn_alignbyte(t[3], t[2], r);
            v.w = __builtin_amdgcn_alignbyte(t[4], t[3], r);
            *reinterpret_cast<uint4*>(dst + b0) = v;
        } else {
            for (int64_t bb = b; bb < e; ++bb) {
                while (bb >= nx) {                           // the next ROI that holds a byte (bb < total <= dst_offs[n])
                    ++lo;
                    o = nx;
                    nx = dst_offs[lo + 1];
                    sp = src + src_offs[idx[lo]];
                }
                dst[bb] = sp[bb - o];
            }
        }
    }
}

}  // namespace

extern "C" int ifcbk_roi_gather(ifcbk_ctx* ctx, const uint8_t* src_pixels, const int64_t* src_offs, const int32_t* src_hs, const int32_t* src_ws,
                                const int64_t* idx, int n, int in_channels, uint8_t* dst_pixels, int64_t dst_capacity, int64_t* dst_offs,
                                int32_t* dst_hs, int32_t* dst_ws, void* stream) {
    if (!ctx) return IFCBK_EINVAL;
    if (n < 1) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_gather: n %d < 1", n);
    if (n > IFCBK_ROI_GATHER_MAX_N) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_gather: n %d > %d, the scan's limit", n, IFCBK_ROI_GATHER_MAX_N);
    if (in_channels != 1 && in_channels != 3) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_gather: in_channels %d is neither 1 nor 3", in_channels);
    if (!src_pixels || !src_offs || !src_hs || !src_ws || !idx || !dst_pixels || !dst_offs || !dst_hs || !dst_ws)
        IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_gather: src_pixels, src_offs, src_hs, src_ws, idx, dst_pixels, dst_offs, dst_hs or dst_ws is NULL");
    if (dst_capacity < 0) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_gather: dst_capacity %lld < 0", (long long)dst_capacity);
    // units of the destination's absolute address that hold a byte of the capacity
    const int64_t units = ((int64_t)((uintptr_t)dst_pixels & 15) + dst_capacity + 15) >> 4;
    const int64_t chunks = (units + GT * GUNITS - 1) / (GT * GUNITS);
    if (chunks > 0x7fffffffll) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_gather: dst_capacity %lld is beyond one grid", (long long)dst_capacity);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(roi_gather_scan_kernel, dim3(1), dim3(GS), 0, st, src_hs, src_ws, idx, n, in_channels, dst_offs, dst_hs, dst_ws);
    IFCBK_LAUNCH_CHECK(ctx, "roi_gather_scan");
    if (chunks > 0) {
        hipLaunchKernelGGL(roi_gather_copy_kernel, dim3((unsigned)chunks), dim3(GT), 0, st, src_pixels, src_offs, idx, n, dst_pixels, dst_capacity,
                           (const int64_t*)dst_offs);
        IFCBK_LAUNCH_CHECK(ctx, "roi_gather_copy");
    }
    return 0;
}
