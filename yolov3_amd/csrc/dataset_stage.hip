// A cached dataset kept in pinned HOST memory, staged into a small device ring one batch at a time (gfx950): the host knows which images a batch needs before any pixel
// is touched (draw_batch), so only those are copied -- by ONE launch per batch that reads the host arena over PCIe and writes
//   * every image of the job table whole into its slot of the ring (a slot is the image's bytes rounded up to 16; the gap bytes are written as zero), and
//   * the image's record of the destination table: the source record with `offset` replaced by the slot's offset in the ring.
// The sampling kernels of dataset.hip / augment.hip then run on (ring, destination table) exactly as they run on (arena, record table) of a device-resident set.
// Images differ in size from a few KB to several MB, so the work is split into chunks of CHUNK bytes: a block copies one chunk and finds its job by bisecting the running
// chunk counts of the job table.  Every load from the host is a PCIe round trip: a lane issues UNROLL independent 16-byte loads before the first use.
// Whatever the job table and the source records hold, no read leaves [host, host + host_bytes) and no write leaves the ring or the destination table: a job that would
// is skipped by every one of its blocks and counted in the status word.
#include "y3_common.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BT = 256;
constexpr int UNROLL = 4;                            // independent 16-byte loads of a lane in flight
constexpr long long PASS = (long long)BT * 16 * UNROLL;   // bytes of one pass of a block (16 KB)
constexpr long long CHUNK = 4 * PASS;                // bytes of one block (64 KB)
constexpr int MAX_JOBS = 8192;                       // images of one launch (a batch of 1024 mixup items draws 8 each)
constexpr int JOB = 3;                               // int64 words of a job: image, slot offset, chunks of the jobs up to and including this one

struct StageArgs {
    const unsigned char* host;     // the device-visible address of the host arena
    long long host_bytes;
    const y3_dataset_image* src;
    long long n_images;
    const long long* jobs;
    int m;
    unsigned char* ring;
    long long ring_bytes;
    y3_dataset_image* dst;
    int* status;
};

// the 16 bytes at position p of an image of `bytes` bytes, with what lies behind the image zeroed
Y3_DEV u32x4 keep_image_bytes(u32x4 v, long long p, long long bytes) {
    const long long left = bytes - p;   // bytes of the vector that belong to the image: 1 .. 15 in the slot's last vector, >= 16 before it
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int l = (int)min(max(left - 4 * q, 0LL), 4LL);   // of dword q
        v[q] &= l == 4 ? ~0u : (1u << (8 * l)) - 1u;
    }
    return v;
}

__global__ __launch_bounds__(BT) void dataset_stage_kernel(const StageArgs a) {
    const long long b = blockIdx.x;
    // the first job whose running chunk count exceeds b (the same search in every lane: uniform loads of a table that stays in L2)
    int lo = 0, hi = a.m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.jobs[(long long)mid * JOB + 2] > b) hi = mid;
        else lo = mid + 1;
    }
    if (lo >= a.m) return;
    const long long* job = a.jobs + (long long)lo * JOB;
    const long long first = lo ? job[2 - JOB] : 0, c = b - first, img = job[0], slot_at = job[1];
    if (c < 0) return;   // (counts that do not ascend: the block belongs to no job)
    bool ok = img >= 0 && img < a.n_images;
    y3_dataset_image r = {};
    long long bytes = 0, slot = 0;
    if (ok) {
        r = a.src[img];
        ok = r.h >= 1 && r.w >= 1 && r.offset >= 0 && (r.offset & 15) == 0 && (long long)r.h * r.w <= a.host_bytes / 3;
    }
    if (ok) {
        bytes = 3LL * r.h * r.w;
        slot = (bytes + 15) & ~15LL;   // (<= host_bytes rounded up to 16 = host_bytes)
        ok = r.offset <= a.host_bytes - bytes && slot_at >= 0 && (slot_at & 15) == 0 && slot <= a.ring_bytes && slot_at <= a.ring_bytes - slot &&
             job[2] - first == (slot + CHUNK - 1) / CHUNK;   // and the job owns exactly the chunks of its slot: none is left uncopied
    }
    if (!ok) {
        if (c == 0 && threadIdx.x == 0) atomicAdd(a.status, 1);
        return;
    }
    const unsigned char* s = a.host + r.offset;   // host_bytes is a multiple of 16: the 16 bytes that hold the image's last byte lie inside the arena
    if (c == 0 && threadIdx.x == 0) {
        r.offset = slot_at;
        a.dst[img] = r;
    }
    const long long end = min((c + 1) * CHUNK, slot);
    unsigned char* d = a.ring + slot_at;
    for (long long p0 = c * CHUNK + (long long)threadIdx.x * 16; p0 < end; p0 += PASS) {
        u32x4 v[UNROLL];
#pragma unroll
        for (int k = 0; k < UNROLL; ++k) {   // all the loads first, none under a branch: a vector past the end re-reads the slot's last one (end >= 16) and is not stored
            const long long p = p0 + (long long)k * BT * 16;
            v[k] = *reinterpret_cast<const u32x4*>(s + min(p, end - 16));
        }
#pragma unroll
        for (int k = 0; k < UNROLL; ++k) {
            const long long p = p0 + (long long)k * BT * 16;
            if (p < end) *reinterpret_cast<u32x4*>(d + p) = keep_image_bytes(v[k], p, bytes);
        }
    }
}

bool aligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

// the device-visible address of [p, p + bytes) if both of its ends are pinned, mapped host memory of one mapping, else null
const unsigned char* mapped_host(const unsigned char* p, long long bytes) {
    hipPointerAttribute_t lo, hi;
    if (hipPointerGetAttributes(&lo, p) != hipSuccess || hipPointerGetAttributes(&hi, p + bytes - 1) != hipSuccess) {
        (void)hipGetLastError();   // (an unregistered address is an error of its own in some runtimes: it is this refusal, not a sticky one)
        return nullptr;
    }
    if (lo.type != hipMemoryTypeHost || hi.type != hipMemoryTypeHost || !lo.devicePointer || !hi.devicePointer) return nullptr;
    if ((const unsigned char*)hi.devicePointer - (const unsigned char*)lo.devicePointer != bytes - 1) return nullptr;
    return (const unsigned char*)lo.devicePointer;
}

}  // namespace

extern "C" int64_t y3_dataset_stage_chunk_bytes(void) { return CHUNK; }

extern "C" int y3_dataset_stage(const uint8_t* host_arena, int64_t host_bytes, const y3_dataset_image* src_images, int64_t n_images, const int64_t* jobs, int32_t m,
                                int64_t n_chunks, uint8_t* ring, int64_t ring_bytes, y3_dataset_image* dst_images, int32_t* status, void* stream) {
    const char* fn = "y3_dataset_stage";
    if (!host_arena || !src_images || !ring || !dst_images || !status || (m > 0 && !jobs)) Y3_FAIL("%s: null argument", fn);
    if (n_images < 1 || n_images > 0x7fffffffLL || m < 0 || m > MAX_JOBS || n_chunks < 0 || n_chunks > 0x7fffffffLL || host_bytes < 16 || (host_bytes & 15) || ring_bytes < 16 ||
        (ring_bytes & 15))
        Y3_FAIL("%s: bad geometry (%lld images in 1 .. 2^31 - 1, %d jobs in 0 .. %d, %lld chunks, a host arena of %lld and a ring of %lld bytes, both positive multiples of 16)", fn,
                (long long)n_images, m, MAX_JOBS, (long long)n_chunks, (long long)host_bytes, (long long)ring_bytes);
    if (!aligned(host_arena, 16) || !aligned(ring, 16)) Y3_FAIL("%s: the host arena and the ring must be 16-byte aligned", fn);
    if (!aligned(src_images, 8) || !aligned(dst_images, 8) || !aligned(jobs, 8) || !aligned(status, 4)) Y3_FAIL("%s: the record tables and the jobs must be 8-byte, the status word 4-byte aligned", fn);
    if (m == 0 || n_chunks == 0) return 0;
    StageArgs a;
    a.host = mapped_host(host_arena, host_bytes);
    if (!a.host) Y3_FAIL("%s: the host arena's %lld bytes are not pinned, mapped host memory", fn, (long long)host_bytes);
    a.host_bytes = host_bytes; a.src = src_images; a.n_images = n_images; a.jobs = (const long long*)jobs; a.m = m;
    a.ring = ring; a.ring_bytes = ring_bytes; a.dst = dst_images; a.status = status;
    hipLaunchKernelGGL(dataset_stage_kernel, dim3((unsigned)n_chunks), dim3(BT), 0, (hipStream_t)stream, a);
    Y3_CHECK_LAUNCH();
    return 0;
}
