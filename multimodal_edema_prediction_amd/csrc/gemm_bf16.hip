// bf16 GEMM front end:  C[M,N] = epilogue( A[M,K] · W[N,K]^T ),  both operands K-contiguous (torch `nn.Linear` layout).
//
// What is decided on the host: the argument checks (once, on MedpGemmArgs), gemm_plan (every dispatch rule and every environment
// switch of the front end, each in one place; DESIGN.md 5.1 shows the rules as a table, with the measurement behind each), the
// dispatcher, the C entry points and the debug hooks.  The kernels: gemm_bf16_tiles.hip (128-row tiles, v3, split-K finish),
// gemm_bf16_v6.hip / gemm_bf16_v7.hip (256 x 256 tiles), gemm_ragged_rows.hip; the launch clock of the tag-1 launches: gemm_profile.hip.
#include "common.h"
#include "gemm_variants.h"
#include "medp_hip.h"

namespace {

int gemm_check_args(const MedpGemmArgs& a, const char* who) {
    MEDP_CHECK_ARG(a.A && a.W && a.C, "%s: null operand", who);
    MEDP_CHECK_ARG(a.M > 0 && a.N > 0 && a.K > 0, "%s: bad shape M=%d N=%d K=%d", who, a.M, a.N, a.K);
    MEDP_CHECK_ARG(a.K % 8 == 0 && a.lda % 8 == 0 && a.ldw % 8 == 0, "%s: K, lda, ldw must be multiples of 8 (16-B chunks)", who);
    MEDP_CHECK_ARG(a.N % 4 == 0 && a.ldc % 4 == 0, "%s: N and ldc must be multiples of 4 (vector epilogue)", who);
    MEDP_CHECK_ARG(a.lda >= a.K && a.ldw >= a.K && a.ldc >= a.N, "%s: leading dimension smaller than the row", who);
    MEDP_CHECK_ARG(!a.residual || a.ldr % 4 == 0, "%s: ldr must be a multiple of 4", who);
    MEDP_CHECK_ARG(((uintptr_t)a.A & 15) == 0 && ((uintptr_t)a.W & 15) == 0 && ((uintptr_t)a.C & 15) == 0,
                   "%s: operands must be 16-byte aligned", who);
    MEDP_CHECK_ARG(a.act == 0 || a.act == 1, "%s: act must be 0 (none) or 1 (gelu)", who);
    return 0;
}

// Which kernel family a GEMM takes and how it is cut.  Values of `kernel` are what medp_dbg_gemm_plan reports.
enum { GEMM_T128x64 = 64, GEMM_T128x128 = 128, GEMM_V3 = 3, GEMM_V6 = 6, GEMM_V7 = 7 };
struct GemmPlan {
    int kernel;
    int nsplit;          // K slices (> 1: split-K through the workspace; 128-row tiles only)
    bool ragged_rows;    // v7 only: the rows past the last full 256-row tile go to a skinny launch of their own
};

// Every dispatch rule, in the order in which it fires.  Pure: reads the shape, the epilogue operands' presence and the switches.
GemmPlan gemm_plan(const MedpGemmArgs& a, int tag, bool has_workspace) {
    static const int variant = medp_env_int("MEDP_GEMM_VARIANT", 0);            // 1 = 128-row tiles, 3 = v3, 6 = v6 (A/B tests)
    static const int splitk = medp_env_int("MEDP_GEMM_SPLITK", -1);             // >= 0: that many K slices wherever a split is considered
    static const int v3_min_tiles = medp_env_int("MEDP_GEMM_V3_MIN_TILES", 192);
    static const int v7_on = medp_env_int("MEDP_GEMM_V7", 1);
    static const int ragged_on = medp_env_int("MEDP_GEMM_RAGGED", 0);
    const int M = a.M, N = a.N, K = a.K;
    // the 256 x 256 tiles (one workgroup per CU) once they occupy most of the chip
    const int tiles256 = ((M + 255) / 256) * ((N + 255) / 256);
    const bool tile256 = M >= 2048 && N >= 256 && (variant == 6 || (variant == 0 && tiles256 >= 160));
    GemmPlan pl{GEMM_T128x128, 1, false};

    // Split-K for SMALL grids (DuETT's skinny GEMMs: 25-100 tiles on 256 CUs): S slices so that tiles x S fills the chip.  Only with
    // a workspace, never for the tagged launches; tiles as the 128-row kernel cuts them; a split pays at 64-127 tiles only for a long K.
    if (has_workspace && tag != 1) {
        const int tiles = ((M + 127) / 128) * (N <= 64 ? (N + 63) / 64 : (N + 127) / 128);
        const int nkt = (K + 63) / 64;
        int S = 1;
        if (splitk >= 0) S = max(1, min(splitk, nkt));
        else if (tiles >= 128 || nkt < 8) S = 1;
        else if (tiles < 64) S = max(1, min(min(256 / tiles, nkt / 4), 16));
        else if (nkt >= 32) S = max(1, min(384 / tiles, nkt / 8));
        if (S > 1) {
            pl.kernel = N <= 64 ? GEMM_T128x64 : GEMM_T128x128;
            pl.nsplit = S;
            return pl;
        }
    }
    if (N <= 64) {
        pl.kernel = GEMM_T128x64;
        return pl;
    }
    if (tile256) {
        // v7: the same K-loop, persistent over the tile list, where the grid is more than one round of workgroups (qkv, fc1)
        const bool v7 = variant != 6 && v7_on && medp_gemm_v7_eligible(a);
        pl.kernel = v7 ? GEMM_V7 : GEMM_V6;
        // MEDP_GEMM_RAGGED=1 (off by default): the rows past the last full 256-row tile (M = 64 * 257: 64 of them) as a skinny launch
        // of their own where that saves v7 a round of workgroups (fc1: 780 tiles = 4 rounds, 768 = 3).  Same bits (gemm_ragged_rows.hip).
        const int rag_rows = M % 256, tiles_n256 = (N + 255) / 256, nfull256 = (M / 256) * tiles_n256;
        if (v7 && ragged_on && rag_rows > 0 && rag_rows <= 128 && nfull256 > 256 && (nfull256 + tiles_n256 + 255) / 256 > (nfull256 + 255) / 256) {
            MedpGemmArgs am = a;
            am.M = M - rag_rows;
            pl.ragged_rows = medp_gemm_v7_eligible(am);
        }
        return pl;
    }
    // v3 (256 x 128 tiles) only where its grid covers most of the chip; MEDP_GEMM_VARIANT=3 forces it for any N > 64
    const int tiles_v3 = ((M + 255) / 256) * ((N + 127) / 128);
    if (variant == 3 || (variant == 0 && M >= 2048 && N >= 256 && tiles_v3 >= v3_min_tiles)) pl.kernel = GEMM_V3;
    return pl;
}

int gemm_launch(const MedpGemmArgs& a, const GemmPlan& pl, int tag, float* workspace, void* stream) {
    switch (pl.kernel) {
    case GEMM_T128x64:
    case GEMM_T128x128:
        return medp_gemm_tile128_launch(a, pl.kernel, tag, pl.nsplit > 1 ? workspace : nullptr, pl.nsplit, stream);
    case GEMM_V3:
        return medp_gemm_v3_launch(a, tag, stream);
    case GEMM_V7: {
        MedpGemmArgs am = a;
        if (pl.ragged_rows) {
            MedpGemmArgs ar = a;
            ar.prof_flags = 2;                 // one clock over both launches: the skinny one stamps the arrival ...
            am.prof_flags = 1;                 // ... the tile kernel the departure
            am.M = a.M - a.M % 256;
            MEDP_TRY(medp_gemm_ragged_rows_launch(ar, am.M, stream));
        }
        const int rc = medp_gemm_v7_launch(am, tag, stream);
        return rc != -1 ? rc : medp_gemm_v6_launch(am, tag, stream);      // (-1: no ticket block left)
    }
    default:
        return medp_gemm_v6_launch(a, tag, stream);
    }
}

// a dense operand-less GEMM of this shape, for the questions that only the plan answers
MedpGemmArgs gemm_shape(int M, int N, int K) {
    return MedpGemmArgs{nullptr, nullptr, nullptr, M, N, K, K, K, N, nullptr, nullptr, nullptr, N, 0, 0, nullptr, 0};
}

}  // namespace

int medp_gemm_run(const MedpGemmArgs& args, int tag, float* workspace, size_t workspace_bytes, void* stream) {
    MEDP_TRY(gemm_check_args(args, "gemm"));
    const GemmPlan pl = gemm_plan(args, tag, workspace != nullptr);
    MEDP_CHECK_ARG(pl.nsplit == 1 || workspace_bytes >= (size_t)pl.nsplit * args.M * args.N * sizeof(float),
                   "gemm: split-K workspace too small (medp_gemm_nt_workspace_bytes)");
    MedpGemmArgs a = args;
    a.prof = nullptr;
    a.prof_flags = 0;
    if (tag != 1 || pl.kernel == GEMM_T128x64) return gemm_launch(a, pl, tag, workspace, stream);
    // the CXR-encoder launches carry the launch clock (the mode-2 slot only into the 256-tile kernels, which stamp it)
    const double flops = 2.0 * (double)a.M * (double)a.N * (double)a.K;
    MEDP_TRY(medp_gemm_profile_begin(pl.kernel == GEMM_V6 || pl.kernel == GEMM_V7, flops, stream, &a.prof));
    const int rc = gemm_launch(a, pl, tag, workspace, stream);
    medp_gemm_profile_end(flops, stream);
    return rc;
}

extern "C" size_t medp_gemm_nt_workspace_bytes(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int S = gemm_plan(gemm_shape(M, N, K), 0, true).nsplit;
    return S > 1 ? (size_t)S * M * N * sizeof(float) : 0;
}

extern "C" int medp_gemm_bf16_nt(const void* A, const void* W, void* C, int M, int N, int K, int lda, int ldw, int ldc,
                                 const float* bias, const float* scale, const float* residual, int ldr, int act, int out_bf16,
                                 void* stream) {
    const MedpGemmArgs a{A, W, C, M, N, K, lda, ldw, ldc, bias, scale, residual, ldr, act, out_bf16, nullptr, 0};
    return medp_gemm_run(a, 0, nullptr, 0, stream);
}

extern "C" int medp_gemm_bf16_nt_ws(const void* A, const void* W, void* C, int M, int N, int K, int lda, int ldw, int ldc,
                                    const float* bias, const float* scale, const float* residual, int ldr, int act, int out_bf16,
                                    float* workspace, size_t workspace_bytes, void* stream) {
    const MedpGemmArgs a{A, W, C, M, N, K, lda, ldw, ldc, bias, scale, residual, ldr, act, out_bf16, nullptr, 0};
    return medp_gemm_run(a, 0, workspace, workspace_bytes, stream);
}

// Debug hook (NOT part of the C ABI in include/medp_hip.h; tests/test_gpu_gemm_buffer_dma.py): ONE launch of a 256-tile kernel on any
// shape, past the grid-size rules of gemm_plan, so that a test reaches every staging path with a few tiles.  kernel 6: one tile
// per workgroup (gemm_bf16_v6.hip; 224-row tiles where its own rule takes them), 7: persistent (gemm_bf16_v7.hip; with
// medp_gemm_persistent_cap below the tile count the workgroups walk several tiles each).
extern "C" int medp_dbg_gemm_tile256(int kernel, const void* A, const void* W, void* C, int M, int N, int K, int lda, int ldw, int ldc,
                                     const float* bias, const float* scale, const float* residual, int ldr, int act, int out_bf16,
                                     void* stream) {
    MEDP_CHECK_ARG(kernel == 6 || kernel == 7, "gemm_tile256: kernel must be 6 or 7");
    const MedpGemmArgs a{A, W, C, M, N, K, lda, ldw, ldc, bias, scale, residual, ldr, act, out_bf16, nullptr, 0};
    MEDP_TRY(gemm_check_args(a, "gemm_tile256"));
    if (kernel == 6) return medp_gemm_v6_launch(a, 0, stream);
    MEDP_CHECK_ARG(medp_gemm_v7_supports(a), "gemm_tile256: the persistent kernel needs a bf16 result, no residual / scale, K %% 128 == 0, K >= 256");
    const int rc = medp_gemm_v7_launch(a, 0, stream);
    MEDP_CHECK_ARG(rc != -1, "gemm_tile256: no ticket block left");
    return rc;
}

// Debug hook (NOT part of the C ABI in include/medp_hip.h; tests/test_gemm_plan_cpu.py): the plan of a shape, out[0] = kernel family
// (64: 128 x 64 tiles, 128: 128 x 128 tiles, 3 / 6 / 7: v3 / v6 / v7), out[1] = K slices, out[2] = ragged rows as their own launch.
// Leading dimensions are K, K, N.  Touches no device.
extern "C" int medp_dbg_gemm_plan(int tag, int M, int N, int K, int has_workspace, int has_residual, int has_scale, int out_bf16,
                                  int* out) {
    MEDP_CHECK_ARG(out && M > 0 && N > 0 && K > 0, "gemm_plan: bad argument");
    static float present;                       // stands for an operand that is there; the plan never reads through it
    MedpGemmArgs a = gemm_shape(M, N, K);
    a.scale = has_scale ? &present : nullptr;
    a.residual = has_residual ? &present : nullptr;
    a.out_bf16 = out_bf16;
    const GemmPlan pl = gemm_plan(a, tag, has_workspace != 0);
    out[0] = pl.kernel;
    out[1] = pl.nsplit;
    out[2] = pl.ragged_rows;
    return 0;
}
