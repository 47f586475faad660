// The host side of the GEMM dispatcher (switch parser, planner, path table: part 1 of csrc/sc_gemm_dispatch.hip) as a
// stand-alone CPU program, for a sanitizer run without a GPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         tools/gemm_plan_host.cpp spatial-clip_amd/csrc/sc_gemm_dispatch.hip -o gemm_plan_host && ./gemm_plan_host
//
// It sweeps sc_debug_gemm_plan over the boundary shapes of tests/_gemmpaths.py under every switch setting and prints how many
// plans it made and how many problems were refused; the sanitizers abort on the first finding.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

extern "C" int sc_debug_gemm_plan(int mode, int epi, int M, int N, int K, int ldc, int splitk, int has_slabs, int colsum,
                                  int slots, int* out, int n);

// what sc_gemm_dispatch.hip calls in the kernel files: the planner reaches none of it
struct GemmPlan;
struct GemmArgs;
struct ReduceOne;
struct ihipStream_t;
#define SC_STUB(name) \
    int name(int, int, const GemmPlan&, const GemmArgs&, ihipStream_t*) { abort(); }
SC_STUB(sc_gemm128_launch) SC_STUB(sc_gemm256_launch) SC_STUB(sc_gemm8p_launch)
int sc_gemm8p_tn_group_launch(const GemmArgs*, int, ihipStream_t*) { abort(); }
int sc_gemm8p_tn_fp8_launch(const GemmArgs&, ihipStream_t*) { abort(); }
int sc_reduce_slabs_launch(const ReduceOne&, int, ihipStream_t*) { abort(); }
int sc_reduce_slabs_group_launch(const ReduceOne*, int, int, ihipStream_t*) { abort(); }
const unsigned* sc_gelu_lut_device(ihipStream_t*, int) { abort(); }
extern "C" long long sc_colsum_ws_floats(int, int) { abort(); }
extern "C" int sc_colsum_bf16(const void*, long long, int, int, float*, float*, void*) { abort(); }

static char last_error[512];
void sc_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}

int main() {
    static const int shapes[][3] = {
        {248, 1024, 128}, {256, 2048, 128}, {2816, 184, 128}, {2816, 192, 128}, {2560, 2560, 136}, {2560, 2560, 128},
        {504, 1024, 128}, {512, 1024, 128}, {2552, 2560, 128}, {2560, 2560, 192}, {2564, 2564, 128}, {2560, 2572, 128},
        {8192, 8192, 192}, {8192, 7936, 192}, {8192, 8192, 128}, {25600, 256, 128}, {25600, 768, 128}, {25600, 1024, 128},
        {6656, 4096, 64}, {6400, 4096, 64}, {6144, 4096, 64}, {6912, 4096, 64}, {2560, 2816, 64}, {2816, 2816, 64},
        {1024, 768, 384}, {1024, 768, 64}, {128, 64, 64}, {8, 8, 8}, {0, 8, 8}, {1 << 30, 1 << 30, 64}};
    static const char* envs[][2] = {{nullptr, nullptr}, {"SC_GEMM_FORCE", "128"}, {"SC_GEMM_FORCE", "256"}, {"SC_GEMM_FORCE", ""},
                                    {"SC_GEMM_SMALL_TILES", "0"}, {"SC_GEMM_SMALL_TILES", "8"}, {"SC_GEMM_SMALL_TILES", "x"},
                                    {"SC_GEMM_PERSIST", "0"}, {"SC_GEMM_PERSIST", ""}, {"SC_GEMM_TAIL", "0"}, {"SC_GEMM_TAIL", "7"},
                                    {"SC_GEMM_TAIL", "1"}, {"SC_GEMM_TAIL", "-5"}, {"SC_GEMM_COLGROUP", "-1:3"},
                                    {"SC_GEMM_COLGROUP", "0:2,8:5,99:4,-7:1,3"}, {"SC_GEMM_COLGROUP", ":"}, {"SC_GEMM_COLGROUP", ""},
                                    {"SC_GELU_LUT", "0"}};
    static const int splitks[] = {-1, 1, 2, 4, 64}, slots[] = {-3, 0, 5, 96, 104, 256};
    long planned = 0, refused = 0;
    for (const auto& e : envs) {
        if (e[0]) setenv(e[0], e[1], 1);
        for (const auto& s : shapes)
            for (int mode = -1; mode <= 2; ++mode)
                for (int epi = -1; epi <= 12; ++epi)
                    for (int sk : splitks)
                        for (int has = 0; has <= 1; ++has)
                            for (int colsum = 0; colsum <= 1; ++colsum)
                                for (int ldc : {s[1], s[1] + 8, 2})
                                    for (int sl : slots) {
                                        int out[8];
                                        for (int n : {8, 3, 0})
                                            (sc_debug_gemm_plan(mode, epi, s[0], s[1], s[2], ldc, sk, has, colsum, sl, out, n) ? refused : planned)++;
                                    }
        if (e[0]) unsetenv(e[0]);
    }
    printf("gemm_plan_host: %ld plans, %ld refusals\n", planned, refused);
    return planned > 0 && refused > 0 ? 0 : 1;
}
