/*
 * sim_zstd_parse.cpp — runs the hash-chain lazy parse of zstd sessions (qatzip_amd/csrc/qzk_zstd_parse.h) on the CPU SIMT
 * emulator (hipsim.h) behind a C ABI for tests/test_sim_zstd_parse.py and tests/golden/gen_zstd_parse.py.  TEST
 * INFRASTRUCTURE, as sim_zstd_seq.cpp.  The launch sequence is that of qzd_zstd_compress_frames_parse (qzd_device.hip): per
 * round of the host plan (qzd_zstd_parse_host.h itself) the head tables zeroed, P1, P2, P3, then P4 without or with the
 * sequence flags; depth 0 runs the kernels of the default parse.
 * With SIM_ZSTD_PARSE_MAIN the file is a program of its own: what a build with -fsanitize=address,undefined runs.
 */
#define QZ_SIM 1
#include "hipsim.h"
#include "../../qatzip_amd/csrc/qzk_zstd_parse.h"
#include "../../qatzip_amd/csrc/qzd_zstd_host.h"
#include "../../qatzip_amd/csrc/qzd_slot_host.h"
#include "../../qatzip_amd/csrc/qzd_zstd_parse_host.h"
#include <vector>

extern "C" {

/* chunks per round of a call, from the host plan */
uint32_t sim_zstd_parse_round(uint32_t block_sz, uint32_t nchunks)
{
    if (!qzd_zs_params_ok(block_sz, 3) || !nchunks) return 0;
    return qzd_zp_plan_for(block_sz, nchunks).batch;
}
/* scratch and slot bytes a chunk of a round takes */
uint64_t sim_zstd_parse_chunk_bytes(uint32_t block_sz)
{
    if (!qzd_zs_params_ok(block_sz, 3)) return 0;
    const qzd_zp_plan P = qzd_zp_plan_for(block_sz, 1);
    return P.chunk_b + P.stride;
}

/* The frames of src under (flags, depth).  round_cap: 0, or fewer chunks per round than the plan's (so that a test sees
 * several rounds of large chunks).  Scratch and slots are filled with 0xEE and have 64 guard bytes behind them.
 * peek (optional, a call of ONE chunk): the chunk's chain distances, then its results (length, distance), n words and 2n
 * words; seqs / lits / counts (optional, ONE chunk): the records (3 words each), the literals, {records, literals}.
 * Returns 0, -1 (out_cap), -2 (parameters), -3 (a frame above its bound, or a store outside scratch and slots). */
int sim_zstd_parse(const uint8_t *src, uint64_t total, uint32_t block_sz, uint32_t mini_match, uint32_t flags, uint32_t depth,
                   uint32_t round_cap, uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *frame_len,
                   uint32_t *peek, uint32_t *seqs_out, uint8_t *lits_out, uint32_t *counts)
{
    if (!qzd_zs_params_ok(block_sz, mini_match) || !qzd_zs_seq_flags_ok(flags) || !qzd_zp_depth_ok(depth)) return -2;
    *out_len = 0;
    if (!total) return 0;
    const uint32_t nb = (uint32_t)((total + block_sz - 1) / block_sz);
    if (depth == 0) {
        if (peek || seqs_out) return -2;
        const uint32_t stride = qzd_zs_stride(block_sz) + 64;
        std::vector<uint8_t> slots((size_t)nb * stride, (uint8_t)0xEE);
        std::vector<uint32_t> lens(nb);
        std::vector<uint8_t> scratch((size_t)nb * QZK_ZS_WAVEB(block_sz) + 64, (uint8_t)0xEE);
        uint32_t counter = 0;
        if (flags)
            sim::launch(nb, 64, 0, [&] { qzk_zstd_pull_seq_kernel(src, total, block_sz, nb, slots.data(), stride, lens.data(), mini_match, &counter, scratch.data(), flags); });
        else
            sim::launch(nb, 64, 0, [&] { qzk_zstd_pull_kernel(src, total, block_sz, nb, slots.data(), stride, lens.data(), mini_match, &counter, scratch.data()); });
        uint64_t run = 0;
        for (uint32_t i = 0; i < nb; i++) {
            if (run + lens[i] > out_cap) return -1;
            memcpy(out + run, slots.data() + (size_t)i * stride, lens[i]);
            if (frame_len) frame_len[i] = lens[i];
            run += lens[i];
        }
        *out_len = run;
        return 0;
    }
    if ((peek || seqs_out) && nb != 1) return -2;
    qzd_zp_plan P = qzd_zp_plan_for(block_sz, nb);
    if (round_cap && round_cap < P.batch) P.batch = round_cap;
    const uint32_t stride = P.stride + 64;
    std::vector<uint8_t> slots((size_t)P.batch * stride), scratch((size_t)P.batch * P.chunk_b + 64);
    std::vector<uint32_t> lens(nb);
    uint64_t run = 0;
    for (uint32_t b = 0; b < nb; b += P.batch) {
        const uint32_t bn = nb - b < P.batch ? nb - b : P.batch;
        const uint64_t boff = (uint64_t)b * block_sz;
        std::fill(slots.begin(), slots.end(), (uint8_t)0xEE);
        std::fill(scratch.begin(), scratch.end(), (uint8_t)0xEE);
        for (uint32_t i = 0; i < bn; i++) memset(scratch.data() + (size_t)i * P.chunk_b, 0, P.head_b);
        uint32_t counter = 0;
        sim::launch(bn, 64, 0, [&] { qzk_zstd_chain_kernel(src + boff, total - boff, block_sz, bn, mini_match, scratch.data()); });
        sim::launch(bn, 64, 0, [&] { qzk_zstd_search_kernel(src + boff, total - boff, block_sz, bn, mini_match, depth, scratch.data()); });
        sim::launch(bn, 64, 0, [&] { qzk_zstd_lazy_kernel(src + boff, total - boff, block_sz, bn, mini_match, depth, scratch.data()); });
        if (peek || seqs_out) {
            const qzk_zp_mem M = qzk_zp_carve(scratch.data(), block_sz, 0);
            if (peek) { memcpy(peek, M.chain, (size_t)total * 4); memcpy(peek + total, M.res, (size_t)total * 8); }
            if (seqs_out) {
                counts[0] = M.meta[0]; counts[1] = M.meta[1];
                memcpy(seqs_out, M.seqs, (size_t)M.meta[0] * 12);
                memcpy(lits_out, M.lits, M.meta[1]);
            }
        }
        if (flags)
            sim::launch(bn, 64, 0, [&] { qzk_zstd_parse_encode_seq_kernel(src + boff, total - boff, block_sz, bn, slots.data(), stride, lens.data() + b, &counter, scratch.data(), flags); });
        else
            sim::launch(bn, 64, 0, [&] { qzk_zstd_parse_encode_kernel(src + boff, total - boff, block_sz, bn, slots.data(), stride, lens.data() + b, &counter, scratch.data()); });
        for (size_t k = (size_t)bn * P.chunk_b; k < scratch.size(); k++) if (scratch[k] != 0xEE) return -3;
        for (uint32_t i = 0; i < bn; i++) {
            const uint32_t c = (uint32_t)(total - boff - (uint64_t)i * block_sz < block_sz ? total - boff - (uint64_t)i * block_sz : block_sz);
            if (lens[b + i] > QZK_ZS_BOUND(c)) return -3;
            for (uint32_t k = QZK_ZS_BOUND(c) + QZK_ZS_SLACK; k < stride; k++) if (slots[(size_t)i * stride + k] != 0xEE) return -3;
            if (run + lens[b + i] > out_cap) return -1;
            memcpy(out + run, slots.data() + (size_t)i * stride, lens[b + i]);
            if (frame_len) frame_len[b + i] = lens[b + i];
            run += lens[b + i];
        }
    }
    *out_len = run;
    return 0;
}

}

#ifdef SIM_ZSTD_PARSE_MAIN
static int fails;
static void run(const char *name, const std::vector<uint8_t> &src, uint32_t block_sz, uint32_t mm, uint32_t flags, uint32_t depth,
                uint32_t round_cap, int expect)
{
    std::vector<uint8_t> out(qzd_zs_bound(src.size(), block_sz) + 64);
    std::vector<uint32_t> fl(src.size() / block_sz + 2);
    uint64_t ol = 0;
    const int rc = sim_zstd_parse(src.data(), src.size(), block_sz, mm, flags, depth, round_cap, out.data(), out.size() - 64, &ol, fl.data(),
                                  NULL, NULL, NULL, NULL);
    if (rc != expect || (rc == 0 && ol > qzd_zs_bound(src.size(), block_sz))) { fprintf(stderr, "%s: rc %d (expected %d), %llu bytes\n", name, rc, expect, (unsigned long long)ol); fails++; }
}
int main()
{
    std::vector<uint8_t> text(70001), ones(131072, (uint8_t)'A'), rnd(5000), far(131072), tiny(1027);
    for (size_t i = 0; i < text.size(); i++) text[i] = i < 3000 ? (uint8_t)(i * 2654435761u >> 13) : (uint8_t)("the quick brown fox "[i % 20] + (i % 977 == 0));
    uint32_t x = 12345;
    for (auto &b : rnd) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
    for (size_t i = 0; i < far.size(); i++) { x = x * 1664525u + 1013904223u; far[i] = i < 70000 ? (uint8_t)(x >> 24) : far[i - 70000]; }
    for (size_t i = 0; i < tiny.size(); i++) tiny[i] = (uint8_t)("abcabcabd"[i % 9]);
    for (uint32_t flags = 0; flags < 4; flags++) {
        run("text", text, 65536, 3, flags, 16, 0, 0);
        run("text mm4", text, 65536, 4, flags, 4, 0, 0);
        run("tiny", tiny, 1024, 3, flags, 64, 1, 0);
    }
    run("ones", ones, 131072, 3, 3, 256, 0, 0);
    run("random", rnd, 1024, 4, 3, 1, 2, 0);
    run("far", far, 131072, 3, 3, 16, 0, 0);
    run("text rounds", text, 1024, 3, 3, 4, 7, 0);
    run("depth 0", text, 65536, 3, 3, 0, 0, 0);
    run("depth 257", text, 65536, 3, 3, 257, 0, -2);
    run("flags 4", text, 65536, 3, 4, 16, 0, -2);
    run("chunk 512", text, 512, 3, 3, 16, 0, -2);
    /* corners of P3 and of a chunk's ends, planted as tests/zstd_parse_traps.py plants them, each in a buffer of exactly its
     * size: the backward extension that stops at p == off (the chunk's first 20 bytes twice), rep1 - 1 == 0 (a run of one
     * byte and a copy at once behind it), a copy with one byte dropped (rep1 - 1 taken), the last mini_match bytes a match,
     * and chunks of 1 .. 4 bytes */
    std::vector<uint8_t> twice(1024), runcopy(1024), dropped(1024), late(1024);
    for (auto *v : { &twice, &runcopy, &dropped, &late }) for (auto &b : *v) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
    for (size_t i = 0; i < 20; i++) twice[20 + i] = twice[i];
    twice[40] = twice[0] ^ 0x55;
    for (size_t i = 600; i < 640; i++) runcopy[i] = runcopy[600];
    runcopy[599] = runcopy[600] ^ 0x55;
    for (size_t i = 0; i < 12; i++) runcopy[640 + i] = runcopy[100 + i];
    for (size_t i = 0; i < 20; i++) dropped[600 + i] = dropped[100 + i];
    for (size_t i = 0; i < 19; i++) dropped[620 + i] = dropped[121 + i];
    for (size_t i = 0; i < 4; i++) late[1020 + i] = late[1015 + i];
    for (uint32_t mm = 3; mm <= 4; mm++)
        for (uint32_t depth : { 1u, 16u, 64u }) {
            run("first bytes twice", twice, 1024, mm, 3, depth, 0, 0);
            run("run and copy", runcopy, 1024, mm, 3, depth, 0, 0);
            run("byte dropped", dropped, 1024, mm, 3, depth, 0, 0);
            run("late match", late, 1024, mm, 3, depth, 0, 0);
            for (size_t n = 1; n <= 4; n++) {
                run("short chunk", std::vector<uint8_t>(n, (uint8_t)7), 1024, mm, depth == 16 ? 0 : 3, depth, 0, 0);
                std::vector<uint8_t> two(twice); two.insert(two.end(), runcopy.begin(), runcopy.begin() + n);
                run("short last chunk", two, 1024, mm, 3, depth, 1, 0);
            }
        }
    /* the plan: a round never passes its budget nor QZD_ZP_ROUND chunks, and always holds one */
    for (uint32_t bs = 1024; bs <= 131072; bs *= 2)
        for (uint32_t nc : { 1u, 2u, 4095u, 4096u, 4097u, 1000000u }) {
            const qzd_zp_plan P = qzd_zp_plan_for(bs, nc);
            if (!P.batch || P.batch > nc || P.batch > QZD_ZP_ROUND || (uint64_t)P.batch * (P.chunk_b + P.stride) > QZD_ZP_BUDGET ||
                P.head_b >= P.chunk_b || (P.chunk_b & 15)) { fprintf(stderr, "plan %u x %u\n", bs, nc); fails++; }
        }
    printf("sim_zstd_parse: %d failures\n", fails);
    return fails ? 1 : 0;
}
#endif
