// Host part of lr_balanced_select (argument checks, scratch layout) as a stand-alone program for a host sanitizer run -- no device, no
// Python:
//   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/select_host_check.hip -o tools/bin/select_host_check -fsanitize=address,undefined && tools/bin/select_host_check
// (`make -C lidarregistration_amd/csrc select_host_check` does both).  csrc/lr_select.hip is compiled into this program as it is; the three
// functions it takes from lr_api.hip are stood in for here, the device check by one that always refuses, so that every path up to the first
// launch runs and nothing is launched.  Exit status 0 and "select_host_check: ok": every check answered as expected, the sanitizers silent.
#include "../lidarregistration_amd/csrc/lr_select.hip"
#include <stdarg.h>
#include <stdlib.h>
#include <vector>

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
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "select_host_check: line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); ++g_failed; } } while (0)

struct call_args {
    int n = 10, n_sessions = 2;
    long long n_draws = 100;
    lr_select_params p;
    const lr_select_params *pp;
    void *fields, *session, *n_cands, *draws, *alive, *n_sel, *out, *res, *scratch;
    size_t bytes = (size_t)1 << 40;
    call_args()
    {
        p.struct_size = sizeof p; p.n_request = 1; p.thresh = 0.1; p.resume = 0; p.max_rounds = 0;
        pp = &p;
        fields = session = n_cands = draws = alive = n_sel = out = res = scratch = (void *)(uintptr_t)256;      // never dereferenced on the host
    }
    int run() const
    {
        return lr_balanced_select((const double *)fields, (const int32_t *)session, (const int32_t *)n_cands, n, n_sessions, (const double *)draws,
                                  n_draws, pp, (uint8_t *)alive, (int32_t *)n_sel, (int32_t *)out, (lr_select_result *)res, scratch, bytes, nullptr);
    }
};

static void refused(const call_args &a, const char *word, int line)
{
    g_err[0] = 0;
    const int before = g_device_checks;
    const int rc = a.run();
    if (rc != LR_EINVAL || !strstr(g_err, word) || g_device_checks != before) {
        fprintf(stderr, "select_host_check: line %d: expected a refusal naming '%s', got %d '%s'\n", line, word, rc, g_err);
        ++g_failed;
    }
}
#define REFUSED(a, word) refused(a, word, __LINE__)

int main()
{
    // the layout: sizes, alignment, monotony, the range of n
    size_t prev = 0;
    for (int n : { 0, 1, 31, 32, 33, 255, 256, 257, 4097, 30000, 1 << 20, SEL_MAX_N }) {
        sel_layout L;
        const size_t total = sel_make_layout(&L, (size_t)n);
        EXPECT(total == lr_balanced_select_scratch_bytes(n));
        EXPECT(total % 256 == 0 && L.part % 256 == 0 && L.pts % 256 == 0 && (L.n_pad * sizeof(double)) % 256 == 0);
        EXPECT(L.n_pad >= (size_t)n && L.n_pad < (size_t)n + 32);
        EXPECT(L.ctl + sizeof(sel_ctl) <= L.part && L.part + (size_t)SEL_PART_BLOCKS * 16 * sizeof(double) <= L.pts);
        EXPECT(L.pts + 6 * L.n_pad * sizeof(double) <= total && total >= prev);
        prev = total;
    }
    EXPECT(lr_balanced_select_scratch_bytes(-1) == 0 && lr_balanced_select_scratch_bytes(SEL_MAX_N + 1) == 0);
    // the rounds a call enqueues
    EXPECT(sel_rounds_needed(0, 5) == 0 && sel_rounds_needed(100, 0) == 0 && sel_rounds_needed(1, 5) == 1);
    EXPECT(sel_rounds_needed(SEL_T, 1) == 2 && sel_rounds_needed(SEL_T + 1, 1) == 3 && sel_rounds_needed(10, 100) == 10);
    EXPECT(sel_rounds_needed(1ll << 40, SEL_MAX_N) == SEL_MAX_N + (1ll << 40) / SEL_T);
    // the refusals, each before the device check
    { call_args a; a.p.struct_size = 16; REFUSED(a, "struct_size"); }
    { call_args a; a.pp = nullptr; REFUSED(a, "null params"); }
    { call_args a; a.n = -1; REFUSED(a, "n must"); }
    { call_args a; a.n = SEL_MAX_N + 1; REFUSED(a, "n must"); }
    { call_args a; a.n_sessions = 0; REFUSED(a, "n_sessions"); }
    { call_args a; a.n_sessions = SEL_MAX_SESSIONS + 1; REFUSED(a, "n_sessions"); }
    for (double t : { 0.0, -0.1, (double)INFINITY, (double)NAN }) { call_args a; a.p.thresh = t; REFUSED(a, "thresh"); }
    { call_args a; a.p.n_request = -1; REFUSED(a, "n_request"); }
    { call_args a; a.p.n_request = 11; REFUSED(a, "n_request"); }
    { call_args a; a.n_draws = -1; REFUSED(a, "n_draws"); }
    { call_args a; a.n_draws = (1ll << 40) + 1; REFUSED(a, "n_draws"); }
    { call_args a; a.p.max_rounds = -1; REFUSED(a, "max_rounds"); }
    { call_args a; a.p.max_rounds = LR_SELECT_MAX_ROUNDS + 1; REFUSED(a, "max_rounds"); }
    { call_args a; a.p.resume = 2; REFUSED(a, "resume"); }
    { call_args a; a.fields = nullptr; REFUSED(a, "fields"); }
    { call_args a; a.session = nullptr; REFUSED(a, "session"); }
    { call_args a; a.n_cands = nullptr; REFUSED(a, "n_cands"); }
    { call_args a; a.draws = nullptr; REFUSED(a, "draws"); }
    { call_args a; a.alive = nullptr; REFUSED(a, "alive"); }
    { call_args a; a.n_sel = nullptr; REFUSED(a, "n_sel"); }
    { call_args a; a.out = nullptr; REFUSED(a, "null out"); }
    { call_args a; a.res = nullptr; REFUSED(a, "result"); }
    { call_args a; a.scratch = nullptr; REFUSED(a, "null scratch"); }
    { call_args a; a.bytes = lr_balanced_select_scratch_bytes(a.n) - 1; REFUSED(a, "scratch too small"); }
    { call_args a; a.scratch = (void *)(uintptr_t)264; REFUSED(a, "aligned"); }
    { call_args a; a.n_draws = 1ll << 30; REFUSED(a, "rounds"); }
    // the rounds are checked before the scratch: too many rounds and a short scratch report the rounds
    { call_args a; a.n_draws = 1ll << 30; a.bytes = lr_balanced_select_scratch_bytes(a.n) - 1; REFUSED(a, "rounds"); }
    // what passes every check reaches the device check, once, and launches nothing: real host buffers, exactly sized
    {
        call_args a;
        std::vector<double> fields(6 * a.n), draws(6 * a.n_draws);
        std::vector<int32_t> session(a.n), n_cands(a.n_sessions, 5), n_sel(a.n_sessions), out(1);
        std::vector<uint8_t> alive(a.n);
        lr_select_result res;
        a.bytes = lr_balanced_select_scratch_bytes(a.n);
        void *raw = malloc(a.bytes + 256);
        a.scratch = (void *)(((uintptr_t)raw + 255) & ~(uintptr_t)255);
        a.fields = fields.data(); a.session = session.data(); a.n_cands = n_cands.data(); a.draws = draws.data(); a.alive = alive.data();
        a.n_sel = n_sel.data(); a.out = out.data(); a.res = &res;
        const int before = g_device_checks;
        EXPECT(a.run() == LR_EINVAL && strstr(g_err, "no device") && g_device_checks == before + 1);
        // the legal corners: nothing requested, no candidate, no draw, a round budget, a resumed call
        a.p.n_request = 0; a.out = nullptr;
        EXPECT(a.run() == LR_EINVAL && g_device_checks == before + 2);
        a.n = 0; a.fields = a.session = a.alive = nullptr; a.n_draws = 0; a.draws = nullptr;
        EXPECT(a.run() == LR_EINVAL && g_device_checks == before + 3);
        call_args b;
        b.scratch = a.scratch; b.n_draws = 1ll << 30; b.p.max_rounds = 64; b.p.resume = 1;
        EXPECT(b.run() == LR_EINVAL && strstr(g_err, "no device") && g_device_checks == before + 4);
        free(raw);
    }
    if (g_failed) { fprintf(stderr, "select_host_check: %d check(s) failed\n", g_failed); return 1; }
    printf("select_host_check: ok\n");
    return 0;
}
