/*
 * sim_zstd_seq.cpp — runs the zstd kernels (qatzip_amd/csrc/qzk_zstd.h) with seq_flags on the CPU SIMT emulator (hipsim.h)
 * behind a C ABI for tests/test_sim_zstd_seq.py and tests/golden/gen_zstd_seq.py.  TEST INFRASTRUCTURE, as sim_zstd.cpp.
 * The launch sequences are those of qzd_zstd_compress_frames_ex / qzd_zstd_encode_frames_ex (qzd_device.hip): flags 0 runs
 * the kernels without flags, anything else the _seq kernels; the host side is qzd_zstd_host.h itself.
 * With SIM_ZSTD_SEQ_MAIN the file is a program of its own that runs hand-made frames under every flag: what a build with
 * -fsanitize=address,undefined runs.
 */
#define QZ_SIM 1
#include "hipsim.h"
#include "../../qatzip_amd/csrc/qzk_zstd.h"
#include "../../qatzip_amd/csrc/qzd_zstd_host.h"
#include <vector>

/* slots filled with 0xEE, 64 guard bytes behind bound + slack that must still be 0xEE afterwards; every frame within its
 * bound: -3 otherwise.  -1: out_cap does not hold the result. */
static int collect(const std::vector<uint8_t> &slots, uint32_t stride, const std::vector<uint32_t> &lens, const std::vector<uint32_t> &content,
                   uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *frame_len)
{
    std::vector<uint64_t> offs(lens.size());
    const uint64_t total = qzd_zs_scan(lens.data(), (uint32_t)lens.size(), offs.data());
    for (size_t i = 0; i < lens.size(); i++) {
        if (lens[i] > QZK_ZS_BOUND(content[i])) return -3;
        for (uint32_t k = QZK_ZS_BOUND(content[i]) + QZK_ZS_SLACK; k < stride; k++) if (slots[i * stride + k] != 0xEE) return -3;
        if (offs[i] + lens[i] > out_cap) return -1;
        memcpy(out + offs[i], slots.data() + i * stride, lens[i]);
        if (frame_len) frame_len[i] = lens[i];
    }
    *out_len = total;
    return 0;
}

extern "C" {

/* sim_zstd with seq_flags.  Returns 0, -1, -2 for bad parameters (a flag bit above 3 among them), -3 (see collect). */
int sim_zstd_ex(const uint8_t *src, uint64_t total, uint32_t block_sz, uint32_t mini_match, uint32_t waves,
                uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *frame_len, uint32_t flags)
{
    if (!qzd_zs_params_ok(block_sz, mini_match) || !qzd_zs_seq_flags_ok(flags)) return -2;
    *out_len = 0;
    if (!total) return 0;
    const uint32_t nb = (uint32_t)((total + block_sz - 1) / block_sz);
    const uint32_t stride = qzd_zs_stride(block_sz) + 64;
    std::vector<uint8_t> slots((size_t)nb * stride, (uint8_t)0xEE);
    std::vector<uint32_t> lens(nb), content(nb);
    for (uint32_t i = 0; i < nb; i++) content[i] = (uint32_t)(total - (uint64_t)i * block_sz < block_sz ? total - (uint64_t)i * block_sz : block_sz);
    uint32_t counter = 0;
    if (!waves || waves > nb) waves = nb;
    std::vector<uint8_t> scratch((size_t)waves * QZK_ZS_WAVEB(block_sz) + 64, (uint8_t)0xEE);
    if (flags)
        sim::launch(waves, 64, 0, [&] { qzk_zstd_pull_seq_kernel(src, total, block_sz, nb, slots.data(), stride, lens.data(), mini_match, &counter, scratch.data(), flags); });
    else
        sim::launch(waves, 64, 0, [&] { qzk_zstd_pull_kernel(src, total, block_sz, nb, slots.data(), stride, lens.data(), mini_match, &counter, scratch.data()); });
    for (size_t k = (size_t)waves * QZK_ZS_WAVEB(block_sz); k < scratch.size(); k++) if (scratch[k] != 0xEE) return -3;
    return collect(slots, stride, lens, content, out, out_cap, out_len, frame_len);
}

/* sim_zstd_encode with seq_flags: -10 for a flag bit above 3 too; -3 also when a wave wrote outside its offset values or
 * the caller's records changed */
int sim_zstd_encode_ex(const uint8_t *lits, const uint32_t *seqs, const uint32_t *desc, uint32_t nframes, uint32_t waves,
                       uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *frame_len, uint32_t flags)
{
    if (!qzd_zs_seq_flags_ok(flags)) return -10;
    *out_len = 0;
    if (!nframes) return 0;
    std::vector<qzk_zs_fdesc> fd(nframes);
    uint32_t maxc = 0;
    uint64_t nseq = 0;
    if (!qzd_zs_describe(desc, nframes, fd.data(), &maxc, &nseq, NULL)) return -10;
    const uint32_t stride = qzd_zs_stride(maxc) + 64;
    std::vector<uint8_t> slots((size_t)nframes * stride, (uint8_t)0xEE);
    std::vector<uint32_t> lens(nframes), content(nframes);
    for (uint32_t i = 0; i < nframes; i++) content[i] = fd[i].content;
    uint32_t counter = 0, bad = 0;
    if (!waves || waves > nframes) waves = nframes;
    if (flags) {
        const std::vector<uint32_t> before(seqs, seqs + 3 * nseq);
        const uint32_t words = qzd_zs_ofv_words(fd.data(), nframes);
        std::vector<uint32_t> ofv((size_t)waves * words + 16, 0xEEEEEEEEu);
        sim::launch(waves, 64, 0, [&] { qzk_zstd_encode_seq_kernel(lits, (const qzk_zs_seq *)seqs, fd.data(), nframes, slots.data(), stride, lens.data(), &bad, &counter, ofv.data(), words, flags); });
        for (size_t k = (size_t)waves * words; k < ofv.size(); k++) if (ofv[k] != 0xEEEEEEEEu) return -3;
        if (memcmp(before.data(), seqs, 12 * nseq)) return -3;
    } else
        sim::launch(waves, 64, 0, [&] { qzk_zstd_encode_kernel(lits, (const qzk_zs_seq *)seqs, fd.data(), nframes, slots.data(), stride, lens.data(), &bad, &counter); });
    if (bad) return -11;
    return collect(slots, stride, lens, content, out, out_cap, out_len, frame_len);
}

}

#ifdef SIM_ZSTD_SEQ_MAIN
/* hand-made frames: `ns` records whose literal length, match length and offset run through small cycles, so that the three
 * tables see few, many and skewed codes and the offsets repeat; every frame under flags 0 .. 3, and the refusals */
static int run_case(uint32_t ns, uint32_t llmod, uint32_t mlmod, uint32_t offmod, uint32_t flags, int expect)
{
    std::vector<uint32_t> seqs;
    std::vector<uint8_t> lits(64, 'x');
    uint32_t content = 64, produced = 64;
    seqs.insert(seqs.end(), { 64u, 3u, 1u });
    content += 3; produced += 3;
    for (uint32_t i = 1; i < ns; i++) {
        const uint32_t ll = (i * 7u) % llmod, ml = 3 + (i * 5u) % mlmod, off = 1 + (i * 3u) % offmod;
        seqs.insert(seqs.end(), { ll, ml, off < produced ? off : 1u });
        for (uint32_t k = 0; k < ll; k++) lits.push_back((uint8_t)(i + k));
        content += ll + ml; produced += ll + ml;
    }
    seqs.insert(seqs.end(), { 0u, 0u, 0u });
    lits.push_back(0);
    const uint32_t desc[3] = { content, ns, (uint32_t)lits.size() - 1 };
    std::vector<uint8_t> out((size_t)content + 12 + 64);
    uint64_t ol = 0; uint32_t fl = 0;
    const int rc = sim_zstd_encode_ex(lits.data(), seqs.data(), desc, 1, 0, out.data(), out.size(), &ol, &fl, flags);
    if (rc != expect) { fprintf(stderr, "case ns=%u flags=%u: rc %d, expected %d\n", ns, flags, rc, expect); return 1; }
    if (rc == 0 && (ol != fl || ol > (uint64_t)content + 12)) { fprintf(stderr, "case ns=%u flags=%u: length %llu\n", ns, flags, (unsigned long long)ol); return 1; }
    return 0;
}
int main()
{
    int fails = 0;
    for (uint32_t flags = 0; flags < 4; flags++) {
        fails += run_case(1, 1, 1, 1, flags, 0);
        fails += run_case(2, 20, 1, 1, flags, 0);
        fails += run_case(64, 5, 7, 3, flags, 0);
        fails += run_case(65, 40, 40, 60, flags, 0);
        fails += run_case(128, 17, 200, 2, flags, 0);
        fails += run_case(700, 70, 100, 50, flags, 0);
        fails += run_case(5000, 12, 9, 4, flags, 0);
    }
    fails += run_case(64, 5, 7, 3, 4, -10);
    /* a chunk through the parse, flags 3: repeated text with a long literal run in front */
    std::vector<uint8_t> src(70001);
    for (size_t i = 0; i < src.size(); i++) src[i] = i < 3000 ? (uint8_t)(i * 2654435761u >> 13) : (uint8_t)("the quick brown fox "[i % 20] + (i % 977 == 0));
    std::vector<uint8_t> out(qzd_zs_bound(src.size(), 65536) + 64);
    uint64_t ol = 0; uint32_t fl[2] = { 0, 0 };
    for (uint32_t flags = 1; flags < 4; flags++) {
        const int rc = sim_zstd_ex(src.data(), src.size(), 65536, 3, 0, out.data(), out.size(), &ol, fl, flags);
        if (rc != 0 || ol != (uint64_t)fl[0] + fl[1] || ol >= src.size()) { fprintf(stderr, "parse flags=%u: rc %d, %llu bytes\n", flags, rc, (unsigned long long)ol); fails++; }
    }
    if (sim_zstd_ex(src.data(), src.size(), 65536, 3, 0, out.data(), out.size(), &ol, fl, 8) != -2) { fprintf(stderr, "flags 8\n"); fails++; }
    printf("sim_zstd_seq: %d failures\n", fails);
    return fails ? 1 : 0;
}
#endif
