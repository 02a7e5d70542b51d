// Host part of lr_nn_wide (argument checks, scratch layout, strip plan) as a stand-alone program for a host sanitizer run -- no device, no
// Python:
//   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/nnw_host_check.hip -o tools/bin/nnw_host_check -fsanitize=address,undefined && tools/bin/nnw_host_check
// (`make -C lidarregistration_amd/csrc nnw_host_check` does both).  csrc/lr_nnw.hip is compiled into this program as it is; the functions it
// takes from lr_api.hip are stood in for here, the device check by one that always refuses, so that every path up to the first launch runs
// and nothing is launched.  This is where the limits n0 = n1 = 2^22, dim = 128 are tested.  Exit status 0 and "nnw_host_check: ok": every
// check answered as expected, the sanitizers silent.
#include "../lidarregistration_amd/csrc/lr_nnw.hip"
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
static int g_device_checks = 0;
int lr_check_memory_device(const void *, hipStream_t, const char *who, int *)
{
    ++g_device_checks;
    lr_set_error("%s: no device in this program", who);
    return LR_EINVAL;
}

static int g_failed = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "nnw_host_check: line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); ++g_failed; } } while (0)

struct call_args {
    int n0 = 100, n1 = 90, dim = 33;
    void *F0, *F1, *idx1, *idx2, *s1, *s2, *scratch;
    size_t bytes = (size_t)1 << 40;
    call_args() { F0 = F1 = idx1 = idx2 = s1 = s2 = scratch = (void *)(uintptr_t)256; }      // never dereferenced on the host
    int run() const
    {
        return lr_nn_wide((const float *)F0, n0, (const float *)F1, n1, dim, (int32_t *)idx1, (int32_t *)idx2, (float *)s1, (float *)s2,
                          scratch, bytes, nullptr);
    }
};

static void refused(const call_args &a, const char *word, int line)
{
    g_err[0] = 0;
    const int before = g_device_checks;
    const int rc = a.run();
    if (rc != LR_EINVAL || !strstr(g_err, word) || g_device_checks != before) {
        fprintf(stderr, "nnw_host_check: line %d: expected a refusal naming '%s', got %d '%s'\n", line, word, rc, g_err);
        ++g_failed;
    }
}
#define REFUSED(a, word) refused(a, word, __LINE__)

int main()
{
    // the layout and the strip plan: sizes, alignment, every tile in exactly one strip, the partials only with more than one strip
    const int sizes[] = { 0, 1, 31, 32, 33, 127, 128, 129, 2049, 4097, 30000, 131072, 131073, 1 << 20, NNW_MAX_N };
    for (int n0 : sizes) for (int n1 : sizes) {
        nnw_layout L;
        const size_t total = nnw_make_layout(&L, (size_t)n0, (size_t)n1);
        EXPECT(total == lr_nn_wide_scratch_bytes(n0, n1, 33) && total == lr_nn_wide_scratch_bytes(n0, n1, 128));
        EXPECT(total >= 256 && total % 256 == 0 && L.nrm0 % 256 == 0 && L.nrm1 % 256 == 0 && L.part % 256 == 0);
        EXPECT(L.nrm0 + (size_t)n0 * 4 <= L.nrm1 && L.nrm1 + (size_t)n1 * 4 <= L.part);
        EXPECT((size_t)L.rblocks * NNW_ROWS >= (size_t)n0 && (size_t)L.tiles * 32 >= (size_t)n1 && (size_t)L.tiles * 32 < (size_t)n1 + 32);
        EXPECT(L.strips >= 1 && L.strips <= NNW_MAX_STRIPS);
        EXPECT((long long)L.strips * L.tiles_per_strip >= L.tiles);
        EXPECT(L.tiles == 0 || (long long)(L.strips - 1) * L.tiles_per_strip < L.tiles);      // the last strip is not empty
        EXPECT((long long)L.rblocks * L.strips <= 0x7fffffffll);
        if (L.strips > 1) EXPECT(L.part + (size_t)n0 * L.strips * sizeof(nnw_part) <= total);
        else EXPECT(L.part <= total);
    }
    {
        nnw_layout L;
        nnw_make_layout(&L, NNW_MAX_N, NNW_MAX_N);
        EXPECT(L.strips == 1 && L.rblocks == NNW_MAX_N / NNW_ROWS && L.tiles == NNW_MAX_N / 32);
        EXPECT((size_t)NNW_MAX_N * NNW_MAX_DIM * sizeof(float) == (size_t)1 << 31);      // the rows' byte offsets need size_t
        nnw_make_layout(&L, 2049, 4097);
        EXPECT(L.strips > 1);
    }
    for (int d = NNW_MIN_DIM; d <= NNW_MAX_DIM; ++d) EXPECT(2 * nnw_steps(d) >= d && nnw_steps(d) <= 64);
    EXPECT(lr_nn_wide_scratch_bytes(-1, 1, 33) == 0 && lr_nn_wide_scratch_bytes(1, NNW_MAX_N + 1, 33) == 0);
    EXPECT(lr_nn_wide_scratch_bytes(1, 1, 32) == 0 && lr_nn_wide_scratch_bytes(1, 1, 129) == 0);
    // the refusals, each before the device check
    for (int d : { 1, 3, 32 }) { call_args a; a.dim = d; REFUSED(a, "use lr_nn_top2"); }
    for (int d : { 0, -1, 129, 1 << 20 }) { call_args a; a.dim = d; REFUSED(a, "33..128"); }
    { call_args a; a.n0 = -1; REFUSED(a, "n0 / n1"); }
    { call_args a; a.n1 = -1; REFUSED(a, "n0 / n1"); }
    { call_args a; a.n0 = NNW_MAX_N + 1; REFUSED(a, "n0 / n1"); }
    { call_args a; a.n1 = NNW_MAX_N + 1; REFUSED(a, "n0 / n1"); }
    { call_args a; a.F0 = nullptr; REFUSED(a, "null F0"); }
    { call_args a; a.F1 = nullptr; REFUSED(a, "null F1"); }
    { call_args a; a.idx1 = nullptr; REFUSED(a, "null idx1"); }
    { call_args a; a.scratch = nullptr; REFUSED(a, "null scratch"); }
    { call_args a; a.bytes = lr_nn_wide_scratch_bytes(a.n0, a.n1, a.dim) - 1; REFUSED(a, "scratch too small"); }
    { call_args a; a.scratch = (void *)(uintptr_t)264; REFUSED(a, "aligned"); }
    // what passes every check reaches the device check, once, and launches nothing: the optional outputs absent, the limits, empty clouds
    {
        call_args a;
        const int before = g_device_checks;
        EXPECT(a.run() == LR_EINVAL && strstr(g_err, "no device") && g_device_checks == before + 1);
        a.idx2 = a.s1 = a.s2 = nullptr;
        EXPECT(a.run() == LR_EINVAL && g_device_checks == before + 2);
        a.n0 = a.n1 = NNW_MAX_N; a.dim = NNW_MAX_DIM; a.bytes = lr_nn_wide_scratch_bytes(a.n0, a.n1, a.dim);
        EXPECT(a.bytes != 0 && a.run() == LR_EINVAL && strstr(g_err, "no device") && g_device_checks == before + 3);
        a.n0 = 0; a.F0 = a.idx1 = nullptr;
        EXPECT(a.run() == LR_EINVAL && g_device_checks == before + 4);
        a.n0 = 5; a.F0 = a.idx1 = a.scratch; a.n1 = 0; a.F1 = nullptr;
        EXPECT(a.run() == LR_EINVAL && g_device_checks == before + 5);
    }
    if (g_failed) { fprintf(stderr, "nnw_host_check: %d check(s) failed\n", g_failed); return 1; }
    printf("nnw_host_check: ok\n");
    return 0;
}
