// rx_bank_abi_harness.cpp -- test infrastructure: the entry points of the two banks of extra receivers (sub-receivers, tuned
// receivers; csrc/ssdr_api.cpp: RxBank) on the paths that return before any device work -- a null ctx, a count over the maximum,
// a null list with a nonzero count, null outputs.  Needs no GPU; every call must RETURN its code.
//
// tests/test_lib_rx_bank_abi.py builds it against libssdr.so and runs it.  For a sanitizer run of the host code, compile it
// together with the library's sources instead (CPU only, never on a GPU):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tests/rx_bank_abi_harness.cpp supersdr_amd/csrc/*.cpp supersdr_amd/csrc/*.hip -o rx_bank_abi_harness
// Prints one line per failed check and "PASS" / "FAIL"; exit code 0 / 1.
#include "../include/ssdr.h"
#include <cstdio>
#include <vector>

static int g_bad = 0;
#define CHECK(expr, want) do { const int rc_ = (expr); if (rc_ != (want)) { printf("FAILED: %s returned %d, not %d\n", #expr, rc_, (int)(want)); g_bad++; } } while (0)

int main()
{
    ssdr_chan_params am;
    CHECK(ssdr_default_params(SSDR_MODE_AM, &am), SSDR_OK);
    std::vector<ssdr_subrx> subs(SSDR_SUBRX_MAX + 1);
    std::vector<ssdr_wb_rx> rx(SSDR_WB_RX_MAX + 1);
    for (uint32_t j = 0; j < subs.size(); j++) subs[j] = ssdr_subrx{j, 0, am};
    for (uint32_t j = 0; j < rx.size(); j++) rx[j] = ssdr_wb_rx{j, 0, 0.0, am};
    uint32_t n = 7;
    ssdr_chan_state st;
    ssdr_chan_consts k;
    ssdr_play_chan pc = {100.0, 0.0};
    std::vector<int16_t> hist(SSDR_HIST * 2), pcm(SSDR_FRAME);
    std::vector<float> taps(SSDR_NTAP_MAX);
    float f[2] = {0.0f, 0.0f}, ms[2];
    uint8_t flag = 0;
    uint32_t launches[2];
    ssdr_ctx *c = nullptr;                                  // (without a GPU there is no other ctx: ssdr_create returns SSDR_ENODEV)
    // the lists: a null ctx with a good list, with a count over the maximum, with a null list and a nonzero count
    CHECK(ssdr_set_subrx(c, subs.data(), 2), SSDR_EINVAL);
    CHECK(ssdr_set_subrx(c, subs.data(), SSDR_SUBRX_MAX + 1), SSDR_EINVAL);
    CHECK(ssdr_set_subrx(c, nullptr, 3), SSDR_EINVAL);
    CHECK(ssdr_set_subrx(c, nullptr, 0), SSDR_EINVAL);
    CHECK(ssdr_set_wb_rx(c, rx.data(), 2), SSDR_EINVAL);
    CHECK(ssdr_set_wb_rx(c, rx.data(), SSDR_WB_RX_MAX + 1), SSDR_EINVAL);
    CHECK(ssdr_set_wb_rx(c, nullptr, 3), SSDR_EINVAL);
    CHECK(ssdr_set_wb_rx(c, nullptr, 0), SSDR_EINVAL);
    CHECK(ssdr_get_subrx(c, subs.data(), &n), SSDR_EINVAL);
    CHECK(ssdr_get_subrx(c, nullptr, nullptr), SSDR_EINVAL);
    CHECK(ssdr_get_wb_rx(c, rx.data(), &n), SSDR_EINVAL);
    CHECK(ssdr_get_wb_rx(c, nullptr, nullptr), SSDR_EINVAL);
    if (n != 7) { printf("FAILED: a refused get wrote the count\n"); g_bad++; }
    // the read-backs, with and without outputs
    CHECK(ssdr_subrx_audio(c, pcm.data(), f, &flag, 0), SSDR_EINVAL);
    CHECK(ssdr_wb_rx_audio(c, nullptr, nullptr, nullptr, 1), SSDR_EINVAL);
    CHECK(ssdr_get_subrx_state(c, 0, 1, &st, hist.data()), SSDR_EINVAL);
    CHECK(ssdr_get_wb_rx_state(c, 0xffffffffu, 0xffffffffu, nullptr, nullptr), SSDR_EINVAL);
    CHECK(ssdr_get_subrx_sam_carrier(c, 0, 1, nullptr, nullptr), SSDR_EINVAL);
    CHECK(ssdr_get_wb_rx_sam_carrier(c, 0, 1, f, f + 1), SSDR_EINVAL);
    CHECK(ssdr_get_subrx_consts(c, 0, 0, &k, taps.data()), SSDR_EINVAL);
    CHECK(ssdr_get_wb_rx_consts(c, 1, 1, nullptr, nullptr), SSDR_EINVAL);
    CHECK(ssdr_run_subrx_playbuffer(c, &pc, pcm.data(), 0), SSDR_EINVAL);
    CHECK(ssdr_run_wb_rx_playbuffer(c, nullptr, nullptr, 0), SSDR_EINVAL);
    CHECK(ssdr_read_wb_rx(c, 0, 1, pcm.data()), SSDR_EINVAL);
    CHECK(ssdr_subrx_stats(c, ms, launches, 1), SSDR_EINVAL);
    CHECK(ssdr_wb_rx_stats(c, ms, ms + 1, launches, 1), SSDR_EINVAL);
    printf(g_bad ? "FAIL\n" : "PASS\n");
    return g_bad ? 1 : 0;
}
