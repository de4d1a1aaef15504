// rx_iq_abi_harness.cpp -- test infrastructure: the entry points of SSDR_MODE_IQ for the extra receivers (ssdr_set_rx_iq,
// ssdr_get_rx_iq, ssdr_subrx_audio_iq, ssdr_wb_rx_audio_iq; csrc/ssdr_api.cpp) on the paths that return before any device work -- a
// null ctx, a bank that is neither 0 nor 1, null outputs -- and the list setters with an SSDR_MODE_IQ row on a null ctx.  Needs no
// GPU; every call must RETURN its code and write nothing.
//
// tests/test_lib_rx_iq_abi.py builds it against libssdr.so and runs it.  For a sanitizer run of the host code, compile it together
// with the library's sources instead (CPU only, never on a GPU):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tests/rx_iq_abi_harness.cpp supersdr_amd/csrc/*.cpp supersdr_amd/csrc/*.hip -o rx_iq_abi_harness
// Prints one line per failed check and "PASS" / "FAIL"; exit code 0 / 1.
#include "../include/ssdr.h"
#include <cstdio>
#include <vector>

static int g_bad = 0;
#define CHECK(expr, want) do { const int rc_ = (expr); if (rc_ != (want)) { printf("FAILED: %s returned %d, not %d\n", #expr, rc_, (int)(want)); g_bad++; } } while (0)

int main()
{
    ssdr_chan_params iq;
    CHECK(ssdr_default_params(SSDR_MODE_IQ, &iq), SSDR_OK);
    if (iq.mode != SSDR_MODE_IQ || iq.low_cut != -5000.0 || iq.high_cut != 5000.0) { printf("FAILED: the mode's defaults\n"); g_bad++; }
    ssdr_ctx *c = nullptr;                                  // (without a GPU there is no other ctx: ssdr_create returns SSDR_ENODEV)
    int on = 7;
    std::vector<int16_t> pairs(2 * SSDR_FRAME, 7);
    // the switch: a null ctx with either bank and either direction, banks that do not exist, a null output
    for (int bank = -1; bank <= 2; bank++) {
        CHECK(ssdr_set_rx_iq(c, bank, 1), SSDR_EINVAL);
        CHECK(ssdr_set_rx_iq(c, bank, 0), SSDR_EINVAL);
        CHECK(ssdr_get_rx_iq(c, bank, &on), SSDR_EINVAL);
        CHECK(ssdr_get_rx_iq(c, bank, nullptr), SSDR_EINVAL);
    }
    CHECK(ssdr_set_rx_iq(c, 0x7fffffff, 1), SSDR_EINVAL);
    CHECK(ssdr_get_rx_iq(c, -0x7fffffff - 1, &on), SSDR_EINVAL);
    if (on != 7) { printf("FAILED: a refused get wrote the flag\n"); g_bad++; }
    // the readers, with and without an output, host and device
    CHECK(ssdr_subrx_audio_iq(c, pairs.data(), 0), SSDR_EINVAL);
    CHECK(ssdr_subrx_audio_iq(c, nullptr, 0), SSDR_EINVAL);
    CHECK(ssdr_subrx_audio_iq(c, nullptr, 1), SSDR_EINVAL);
    CHECK(ssdr_wb_rx_audio_iq(c, pairs.data(), 0), SSDR_EINVAL);
    CHECK(ssdr_wb_rx_audio_iq(c, nullptr, 1), SSDR_EINVAL);
    for (int16_t v : pairs)
        if (v != 7) { printf("FAILED: a refused reader wrote its output\n"); g_bad++; break; }
    // the list setters with a row in the mode: the null ctx is what they answer
    ssdr_subrx sub = {1, 0, iq};
    ssdr_wb_rx rx = {1, 0, 0.0, iq};
    CHECK(ssdr_set_subrx(c, &sub, 1), SSDR_EINVAL);
    CHECK(ssdr_set_wb_rx(c, &rx, 1), SSDR_EINVAL);
    printf(g_bad ? "FAIL\n" : "PASS\n");
    return g_bad ? 1 : 0;
}
