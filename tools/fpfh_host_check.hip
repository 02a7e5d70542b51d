// Host part of lr_fpfh (argument checks, scratch layout) as a stand-alone program for a host sanitizer run -- no device, no Python:
//   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/fpfh_host_check.hip -o tools/bin/fpfh_host_check -fsanitize=address,undefined && tools/bin/fpfh_host_check
// (`make -C lidarregistration_amd/csrc fpfh_host_check` does both).  csrc/lr_fpfh.hip and csrc/lr_nn3.hip (the grid it runs on) are compiled
// into this program as they are; the functions they take from lr_api.hip are stood in for here, the device check by one that always
// refuses, so that every path up to the first launch runs and nothing is launched.  This is where the limits n = 2^22, max_nn = 128 are
// tested.  Exit status 0 and "fpfh_host_check: ok": every check answered as expected, the sanitizers silent.
#include "../lidarregistration_amd/csrc/lr_nn3.hip"
#include "../lidarregistration_amd/csrc/lr_fpfh.hip"
#include <stdarg.h>
#include <stdlib.h>

static char g_err[512];
void lr_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
extern "C" int lr_version(void) { return 103; }
static int g_device_checks = 0;
int lr_check_memory_device(const void *, hipStream_t, const char *who, int *)
{
    ++g_device_checks;
    lr_set_error("%s: no device in this program", who);
    return LR_EINVAL;
}

static int g_failed = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "fpfh_host_check: line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); ++g_failed; } } while (0)

struct call_args {
    int n = 100, max_nn = 100;
    double radius = 1.5;
    void *xyz, *nrm, *o64, *o32, *info, *scratch;
    size_t bytes = (size_t)1 << 42;
    call_args() { xyz = nrm = o64 = o32 = info = scratch = (void *)(uintptr_t)256; }      // never dereferenced on the host
    int run() const
    {
        return lr_fpfh((const double *)xyz, (const double *)nrm, n, radius, max_nn, (double *)o64, (float *)o32, (int32_t *)info, scratch, bytes, nullptr);
    }
};

static void refused(const call_args &a, const char *word, int line)
{
    g_err[0] = 0;
    const int before = g_device_checks;
    const int rc = a.run();
    if (rc != LR_EINVAL || !strstr(g_err, word) || g_device_checks != before) {
        fprintf(stderr, "fpfh_host_check: line %d: expected a refusal naming '%s', got %d '%s'\n", line, word, rc, g_err);
        ++g_failed;
    }
}
#define REFUSED(a, word) refused(a, word, __LINE__)

int main()
{
    // the layout: the grid's arena first, then the lengths, the lists and the SPFH rows, each 256-byte aligned and large enough
    size_t prev = 0;
    for (int n : { 0, 1, 2, 257, 3000, 75000, 1 << 20, NN_MAX_N })
        for (int k : { FP_MIN_NN, 100, FP_MAX_NN }) {
            fp_layout L;
            nn_layout G;
            const size_t total = fp_make_layout(&L, (size_t)n, (size_t)k), m = n > 0 ? (size_t)n : 1;
            EXPECT(total == lr_fpfh_scratch_bytes(n, k) && total == L.end && total % 256 == 0);
            EXPECT(L.nn == 0 && L.cnt % 256 == 0 && L.lists % 256 == 0 && L.spfh % 256 == 0);
            EXPECT(L.cnt >= nn_make_layout(&G, (size_t)n, (size_t)n, 0) && L.cnt >= lr_nn3_scratch_bytes(n, n));
            EXPECT(L.cnt + m * 4 <= L.lists && L.lists + m * (size_t)k * 4 <= L.spfh && L.spfh + m * FP_BINS * 8 <= L.end);
            if (k == FP_MAX_NN) { EXPECT(total >= prev); prev = total; }
        }
    {
        fp_layout L;
        fp_make_layout(&L, NN_MAX_N, FP_MAX_NN);
        EXPECT(L.spfh - L.lists >= ((size_t)1 << 31));          // the lists alone reach 2^31 bytes, the SPFH rows lie behind them: size_t offsets
        EXPECT(L.end > ((size_t)3 << 30));
    }
    EXPECT(lr_fpfh_scratch_bytes(-1, 100) == 0 && lr_fpfh_scratch_bytes(NN_MAX_N + 1, 100) == 0);
    EXPECT(lr_fpfh_scratch_bytes(10, 1) == 0 && lr_fpfh_scratch_bytes(10, FP_MAX_NN + 1) == 0);
    // the refusals, each before the device check
    for (double r : { 0.0, -1.0, (double)INFINITY, (double)NAN, 1e200 }) { call_args a; a.radius = r; REFUSED(a, "radius"); }
    { call_args a; a.max_nn = 1; REFUSED(a, "max_nn"); }
    { call_args a; a.max_nn = FP_MAX_NN + 1; REFUSED(a, "max_nn"); }
    { call_args a; a.n = -1; REFUSED(a, "n must"); }
    { call_args a; a.n = NN_MAX_N + 1; REFUSED(a, "n must"); }
    { call_args a; a.xyz = nullptr; REFUSED(a, "null xyz"); }
    { call_args a; a.nrm = nullptr; REFUSED(a, "null normals"); }
    { call_args a; a.o64 = a.o32 = nullptr; REFUSED(a, "null out_f64 and out_f32"); }
    { call_args a; a.info = nullptr; REFUSED(a, "null info"); }
    { call_args a; a.scratch = nullptr; REFUSED(a, "null scratch"); }
    { call_args a; a.bytes = lr_fpfh_scratch_bytes(a.n, a.max_nn) - 1; REFUSED(a, "scratch too small"); }
    { call_args a; a.scratch = (void *)(uintptr_t)264; REFUSED(a, "aligned"); }
    // what passes every check reaches the device check, once, and launches nothing: either output absent, the limits, an empty cloud
    {
        call_args a;
        const int before = g_device_checks;
        EXPECT(a.run() == LR_EINVAL && strstr(g_err, "no device") && g_device_checks == before + 1);
        a.o64 = nullptr;
        EXPECT(a.run() == LR_EINVAL && g_device_checks == before + 2);
        a.o64 = a.o32; a.o32 = nullptr;
        EXPECT(a.run() == LR_EINVAL && g_device_checks == before + 3);
        a.n = NN_MAX_N; a.max_nn = FP_MAX_NN; a.bytes = lr_fpfh_scratch_bytes(a.n, a.max_nn);
        EXPECT(a.bytes != 0 && a.run() == LR_EINVAL && strstr(g_err, "no device") && g_device_checks == before + 4);
        a.n = 0; a.xyz = a.nrm = a.o64 = nullptr;
        EXPECT(a.run() == LR_EINVAL && g_device_checks == before + 5);
    }
    if (g_failed) { fprintf(stderr, "fpfh_host_check: %d check(s) failed\n", g_failed); return 1; }
    printf("fpfh_host_check: ok\n");
    return 0;
}
