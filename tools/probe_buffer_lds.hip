// Stand-alone probe (its own main, not part of libmedp_hip.so): what a raw buffer LDS-DMA load (`buffer_load_dwordx4 ... offen lds`)
// does on gfx950 with lanes past the descriptor's num_records, and whether the scalar offset takes part in that range check.
// The block GEMMs' staging (gemm_tile256.h) relies on the answers; profiles/r05_gemm_buffer_dma.txt records them.
//
//     hipcc --offload-arch=gfx950 -O2 tools/probe_buffer_lds.hip -o probe_buffer_lds && ./probe_buffer_lds
//
// One wave.  The source is 4 KiB in the middle of a 64-KiB allocation (dword i of the allocation holds i + 1, so no access the
// probe can make leaves the allocation); LDS is filled with 0xAAAAAAAA before every case.  Each case stages one piece (lane l
// asks for 16 bytes at voffset(l) + soffset) and copies the wave's 1 KiB of LDS out.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define CHECK(e)                                                                             \
    do {                                                                                     \
        hipError_t e__ = (e);                                                                \
        if (e__ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(e__)); return 2; } \
    } while (0)

constexpr int NCASE = 6;
constexpr uint32_t FILL = 0xAAAAAAAAu;

struct Case { unsigned records, vbase, soff; };

__global__ __launch_bounds__(64) void probe_kernel(const uint32_t* src, uint32_t* out, const Case c0, const Case c1, const Case c2, const Case c3, const Case c4, const Case c5) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[256];
    const int lane = threadIdx.x;
    const Case cs[NCASE] = {c0, c1, c2, c3, c4, c5};
#pragma unroll
    for (int c = 0; c < NCASE; ++c) {
        for (int i = 0; i < 4; ++i) lds[lane * 4 + i] = FILL;
        __syncthreads();
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)cs[c].records, 0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, cs[c].vbase + lane * 16, cs[c].soff, 0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int i = 0; i < 4; ++i) out[c * 256 + lane * 4 + i] = lds[lane * 4 + i];
        __syncthreads();
    }
}

int main() {
    const int NALLOC = 16384, MID = 8192;                  // dwords; the descriptor's base is dword MID
    uint32_t* h = (uint32_t*)malloc(NALLOC * 4);
    for (int i = 0; i < NALLOC; ++i) h[i] = i + 1;
    uint32_t *d, *o;
    CHECK(hipMalloc(&d, NALLOC * 4));
    CHECK(hipMalloc(&o, NCASE * 1024));
    CHECK(hipMemcpy(d, h, NALLOC * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(o, 0xff, NCASE * 1024));
    const Case cases[NCASE] = {
        {1024, 0, 0},      // all 64 lanes in range
        {512, 0, 0},       // lanes 32-63 past num_records through the vector offset
        {0, 0, 0},         // no records at all
        {512, 0, 256},     // lanes 16-31: vector offset in range, vector + scalar offset past num_records
        {512, 256, 0},     // the same addresses through the vector offset alone (control)
        {520, 0, 0},       // lane 32: its first 8 bytes in range, the rest not
    };
    const char* what[NCASE] = {"records 1024, voff 16 l", "records 512, voff 16 l", "records 0", "records 512, voff 16 l, soff 256",
                               "records 512, voff 256 + 16 l", "records 520, voff 16 l"};
    probe_kernel<<<1, 64>>>(d + MID, o, cases[0], cases[1], cases[2], cases[3], cases[4], cases[5]);
    CHECK(hipDeviceSynchronize());
    uint32_t* r = (uint32_t*)malloc(NCASE * 1024);
    CHECK(hipMemcpy(r, o, NCASE * 1024, hipMemcpyDeviceToHost));
    for (int c = 0; c < NCASE; ++c) {
        // per lane: L = live data (dword of the source at voffset + soffset), Z = zeros, U = LDS untouched, ? = anything else
        char line[65];
        for (int l = 0; l < 64; ++l) {
            int live = 0, zero = 0, fill = 0;
            for (int i = 0; i < 4; ++i) {
                const uint32_t v = r[c * 256 + l * 4 + i];
                const uint32_t want = MID + (cases[c].vbase + cases[c].soff) / 4 + l * 4 + i + 1;
                live += v == want;
                zero += v == 0;
                fill += v == FILL;
            }
            line[l] = live == 4 ? 'L' : zero == 4 ? 'Z' : fill == 4 ? 'U' : '?';
        }
        line[64] = 0;
        printf("case %d (%-34s): %s\n", c, what[c], line);
        if (c == 5) printf("        lane 32 dwords: %08x %08x %08x %08x (live would be %08x ...)\n", r[c * 256 + 128], r[c * 256 + 129], r[c * 256 + 130],
                           r[c * 256 + 131], MID + 128 + 1);
    }
    const char b = ({ char x = 'U'; for (int l = 32; l < 64; ++l) if (r[1 * 256 + l * 4] == 0) x = 'Z'; x; });
    const bool soff_checked = r[3 * 256 + 16 * 4] != (uint32_t)(MID + 64 + 16 * 4 + 1);
    printf("(a) the scalar offset %s part in the num_records check\n", soff_checked ? "TAKES" : "takes NO");
    printf("(b) an out-of-range lane of a buffer LDS-DMA load %s\n", b == 'Z' ? "writes ZEROS to LDS" : "leaves LDS UNTOUCHED");
    return 0;
}
