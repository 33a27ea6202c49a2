// demod_streams_push's staging (audio-network_amd/csrc/stream_stage.h: the
// batch layout, a stream's carry + packet into its run, the new carry, the
// rollback) against a naive model, on the host alone. The model concatenates
// a stream's old carry with the mono view of its packet, slices windows at
// hop and keeps the samples from W hop onward. Packets, runs and carries are
// exact-size heap allocations, so ASan sees any access past them; UBSan the
// arithmetic. Exit 0 = OK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../audio-network_amd/csrc/stream_stage.h"

namespace {

using Samples = std::vector<int16_t>;

[[noreturn]] void fail(const char *what, size_t n, size_t hop, int ch, int mode, size_t lead, size_t S,
                       int push, size_t s)
{
    std::printf("FAIL %s: n %zu hop %zu channels %d mode %d lead_in %zu streams %zu push %d stream %zu\n",
                what, n, hop, ch, mode, lead, S, push, s);
    std::exit(1);
}

// the model's mono view, written out on its own
Samples model_mono(int channels, int mode, const int16_t *pcm, size_t frames)
{
    Samples m(frames);
    for (size_t i = 0; i < frames; ++i) {
        if (channels == 1) m[i] = pcm[i];
        else if (mode == DEMOD_CH_LEFT) m[i] = pcm[2 * i];
        else if (mode == DEMOD_CH_RIGHT) m[i] = pcm[2 * i + 1];
        else m[i] = (int16_t)(((int)pcm[2 * i] + (int)pcm[2 * i + 1]) >> 1);
    }
    return m;
}

struct Stream {
    std::unique_ptr<int16_t[]> carry;   // n - 1 samples: a carry is always shorter than a window
    size_t len = 0, skip = 0;
    Samples model;                      // the model's carry
};

size_t g_branch_packet = 0, g_branch_carry = 0, g_gaps = 0, g_rollbacks = 0;

void run_case(size_t n, size_t hop, int channels, int mode, size_t lead, size_t S, std::mt19937 &rng)
{
    demod_cfg_t c;
    std::memset(&c, 0, sizeof(c));
    c.n = (uint32_t)n;
    c.hop = (uint32_t)hop;
    c.channels = (uint32_t)channels;
    c.channel_mode = mode;
    const size_t lens[6] = {0, 1, n - 1, n, n + hop - 1, 3 * n + 7};
    std::vector<Stream> st(S);
    for (Stream &x : st) {
        x.carry.reset(new int16_t[n - 1]);
        x.skip = lead;
    }
    for (int push = 0; push < 8; ++push) {
#define FAIL(what, s) fail(what, n, hop, channels, mode, lead, S, push, s)
        // packets (exact size), and what the model makes of them
        std::vector<std::unique_ptr<int16_t[]>> pcm(S);
        std::vector<size_t> frames(S), fresh(S), have(S), total(S);
        std::vector<Samples> cat(S);
        for (size_t s = 0; s < S; ++s) {
            frames[s] = lens[rng() % 6];
            pcm[s].reset(new int16_t[frames[s] * channels]);
            for (size_t i = 0; i < frames[s] * channels; ++i) pcm[s][i] = (int16_t)(rng() & 0xFFFF);
            const size_t drop = std::min(st[s].skip, frames[s]);
            fresh[s] = frames[s] - drop;
            have[s] = st[s].len;
            total[s] = have[s] + fresh[s];
            cat[s] = st[s].model;
            const Samples m = model_mono(channels, mode, pcm[s].get() + drop * channels, fresh[s]);
            cat[s].insert(cat[s].end(), m.begin(), m.end());
            if (have[s] != st[s].model.size()) FAIL("carry length before the push", s);
        }
        // the layout
        std::vector<size_t> first(S, ~(size_t)0), w(S);
        std::vector<uint32_t> counts(S, ~0u);
        size_t W = ~(size_t)0;
        const size_t Wb = fskd::run_layout(S, n, hop, [&](size_t s) { return total[s]; }, first.data(),
                                           counts.data(), &W);
        size_t mW = 0, mWb = 0;
        for (size_t s = 0; s < S; ++s) {
            size_t mw = 0;
            while (mw * hop + n <= cat[s].size()) ++mw;   // windows sliced at hop
            w[s] = mw;
            if (fskd::windows_for(total[s], n, hop) != mw || counts[s] != mw) FAIL("window count", s);
            if (first[s] != mWb) FAIL("first[]", s);
            mW += mw;
            size_t slots = 0;
            while (mw && slots * hop < (mw - 1) * hop + n) ++slots;   // hops that cover the run
            mWb += slots;
        }
        if (W != mW || Wb != mWb) FAIL("W / Wb", 0);
        // staging into a run buffer of exactly Wb hops
        std::unique_ptr<int16_t[]> runs(new int16_t[Wb * hop]);
        for (size_t i = 0; i < Wb * hop; ++i) runs[i] = 0x5A5A;
        auto stage_all = [&] {
            for (size_t s = 0; s < S; ++s)
                st[s].len = fskd::stage_stream(c, fresh[s] ? pcm[s].get() + (frames[s] - fresh[s]) * channels : nullptr,
                                               fresh[s], st[s].carry.get(), have[s], runs.get() + first[s] * hop);
        };
        stage_all();
        if (push % 3 == 1) {
            // a failed batch: every carry comes back from the runs, then the push is made again
            for (size_t s = 0; s < S; ++s) {
                st[s].len = fskd::unstage_stream(c, fresh[s], st[s].carry.get(), have[s],
                                                 runs.get() + first[s] * hop);
                if (st[s].len != st[s].model.size() ||
                    (st[s].len && std::memcmp(st[s].carry.get(), st[s].model.data(), st[s].len * 2)))
                    FAIL("rollback", s);
            }
            ++g_rollbacks;
            stage_all();
        }
        for (size_t s = 0; s < S; ++s) {
            const size_t nxt = s + 1 < S ? first[s + 1] : Wb;
            const int16_t *b = runs.get() + first[s] * hop;
            const size_t L = w[s] ? (w[s] - 1) * hop + n : 0, span = (nxt - first[s]) * hop;
            for (size_t i = 0; i < span; ++i)
                if (b[i] != (i < L ? cat[s][i] : 0)) FAIL(i < L ? "run samples" : "gap fill", s);
            for (size_t j = 0; j < w[s]; ++j)   // batch window first[s] + j is the stream's window j
                if (std::memcmp(runs.get() + (first[s] + j) * hop, cat[s].data() + j * hop, n * 2))
                    FAIL("window", s);
            if (span > L) ++g_gaps;
            if (w[s]) ++(w[s] * hop >= have[s] ? g_branch_packet : g_branch_carry);
            // a stream without a window keeps its frames (the push's tail)
            if (!w[s] && fresh[s]) {
                fskd::mono_frames(c, pcm[s].get() + (frames[s] - fresh[s]) * channels, fresh[s],
                                  st[s].carry.get() + have[s]);
                st[s].len = total[s];
            }
            st[s].model.assign(cat[s].begin() + w[s] * hop, cat[s].end());
            if (st[s].len != st[s].model.size() ||
                (st[s].len && std::memcmp(st[s].carry.get(), st[s].model.data(), st[s].len * 2)))
                FAIL("new carry", s);
            st[s].skip -= std::min(st[s].skip, frames[s]);
        }
#undef FAIL
    }
}

}  // namespace

int main()
{
    std::mt19937 rng(20240607u);
    const size_t shapes[4][2] = {{64, 8}, {64, 24}, {64, 64}, {128, 64}};
    const int chans[4][2] = {{1, DEMOD_CH_LEFT}, {2, DEMOD_CH_LEFT}, {2, DEMOD_CH_RIGHT}, {2, DEMOD_CH_DOWNMIX}};
    size_t cases = 0;
    for (const auto &sh : shapes)
        for (const auto &ch : chans)
            for (size_t lead : {(size_t)0, (size_t)5, 3 * sh[0] + 20})   // the last: past any first packet
                for (size_t S : {1, 3, 9}) {
                    run_case(sh[0], sh[1], ch[0], ch[1], lead, S, rng);
                    ++cases;
                }
    if (!g_branch_packet || !g_branch_carry || !g_gaps || !g_rollbacks) {
        std::printf("FAIL coverage: carry from the packet %zu, from the old carry %zu, gaps %zu, rollbacks %zu\n",
                    g_branch_packet, g_branch_carry, g_gaps, g_rollbacks);
        return 1;
    }
    std::printf("stream stage OK: %zu cases, carry from the packet %zu / from the old carry %zu, %zu gaps, "
                "%zu rollbacks\n", cases, g_branch_packet, g_branch_carry, g_gaps, g_rollbacks);
    return 0;
}
