/*
 * tests/streamcheck_main.cpp -- CPU driver for the streamed-code form of the k = 4 pair-table interpreter
 * (k_ll_fused4_v4s; op words, stream layout and replay check in phyly_amd/csrc/plk_program.h), built with
 * AddressSanitizer + UBSan by tests/test_k4_stream_host.py.
 *
 * Over the seeded random trees of tests/progcheck_main.cpp (same generator, same seed, same 6000 iterations; the trees the
 * pair-table interpreter does not take -- more than 4 stack slots, no observed node, tables beyond the LDS -- are
 * skipped) it builds the pair-table program, the streamed op words and a host image of the code stream for a random
 * code matrix, with nchar in {4, 5, 16}, C in {1, 4} and S in {1, 129, 300} rotating over the iterations, and
 *   - replays the interpreter's fetches on the image, lane by lane and site half by site half: the prologue's three
 *     loads, every ADVANCE's load (all inside the allocation, which is exactly the stream: ASan watches too) and
 *     every observation op's extraction, which must deliver the byte the PROGRAM's next observation op needs
 *     (code, or code(b) * nchar + code(c) for a cherry), worked out from the program and the codes alone;
 *   - requires plk_fused_check_v4s to accept, and to reject corrupted streams: a wrong byte position, a missing spare
 *     chunk, a table field past the image, an ADVANCE of the wrong kind.
 * Prints "ok <trees taken> <observations replayed>" and exits 0, or the first failure and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "plk_program.h"

struct Tree { int N; std::vector<int> ip, ix, pre; };

/* as in progcheck_main.cpp */
static bool make_tree(int N, const std::vector<int> &ea, const std::vector<int> &eb, Tree &t)
{
    t.N = N; t.ip.assign(N + 1, 0); t.ix.assign(N > 1 ? N - 1 : 1, 0); t.pre.clear();
    std::vector<int> indeg(N, 0);
    for (int e = 0; e < N - 1; e++) { t.ip[ea[e] + 1]++; indeg[eb[e]]++; }
    for (int a = 0; a < N; a++) t.ip[a + 1] += t.ip[a];
    std::vector<int> fill(t.ip.begin(), t.ip.end() - 1);
    for (int e = 0; e < N - 1; e++) t.ix[fill[ea[e]]++] = eb[e];
    int root = -1;
    for (int a = 0; a < N; a++) if (!indeg[a]) { if (root >= 0) return false; root = a; }
    if (root < 0) return false;
    t.pre.push_back(root);
    for (size_t h = 0; h < t.pre.size(); h++)
        for (int idx = t.ip[t.pre[h]]; idx < t.ip[t.pre[h] + 1]; idx++) t.pre.push_back(t.ix[idx]);
    return (int)t.pre.size() == N;
}

static long g_taken = 0, g_obs = 0;

static std::string check_tree(const Tree &t, const std::vector<char> &has, int nchar, int C, long S, std::mt19937_64 &crng)
{
    const int N = t.N;
    PlkProgram pg;
    plk_program_build(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
    if (pg.slots_needed > 4 || pg.obs_nodes.empty()) return "";
    PlkFusedPT fp;
    plk_fused_pt_build(N, t.ip.data(), t.ix.data(), pg, nchar, 1 << 30, fp, true);
    const unsigned tip_base = 0;
    const size_t lds = plk_fused_v4s_lds_bytes(fp, nchar, C);
    if (lds > plk_pt_lds_limit(1024) || lds / 32 >= 65536 || fp.units >= 2048 || fp.row_node.size() >= 65536) return "";
    std::string bad = plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, fp, nchar, 1, 0, true, false);
    if (!bad.empty()) return "32-bit program: " + bad;
    PlkFusedV4S vs;
    plk_fused_v4s_words(fp, nchar, C, tip_base, vs);
    bad = plk_fused_check_v4s(fp, vs, nchar, C, tip_base, lds);
    if (!bad.empty()) return bad;
    g_taken++;

    /* what the program's observation ops need, from the program alone: node (and second node of a cherry) per observation */
    std::vector<int> need_b, need_c;
    for (size_t pc = 0; pc < pg.ops.size(); pc++) {
        const int code = pg.ops[pc].x & 0xff;
        if (code == OP_TIP_SET && plk_pair_at(N, t.ip.data(), t.ix.data(), pg, pc)) { need_b.push_back(pg.ops[pc].y); need_c.push_back(pg.ops[pc + 1].y); pc += 2; }
        else if (code == OP_TIP_SET || code == OP_TIP_MUL || code == OP_NODE_MUL) { need_b.push_back(pg.ops[pc].y); need_c.push_back(-1); }
    }
    const int nobs = (int)need_b.size();
    if (nobs != vs.nobs) return "the stream has " + std::to_string(vs.nobs) + " observations, the program " + std::to_string(nobs);

    /* code rows [N][Spad], zero padded like the engine's; the stream image exactly as large as the engine allocates */
    const size_t Spad = (size_t)(S + 3071) / 3072 * 3072;
    std::vector<uint8_t> codes((size_t)N * Spad, 0);
    for (int a = 0; a < N; a++) for (long s = 0; s < S; s++) codes[(size_t)a * Spad + s] = (uint8_t)(crng() % (unsigned)nchar);
    std::vector<int> rn(fp.row_node);
    rn.insert(rn.end(), fp.row_node2.begin(), fp.row_node2.end());
    const int nrows = (int)fp.row_node.size();
    const size_t nunits = (size_t)(S + PLK_V4S_UNIT - 1) / PLK_V4S_UNIT;
    const size_t total = nunits * vs.chunks * PLK_V4S_UNIT;
    std::vector<unsigned> image(total);
    for (size_t u = 0; u < nunits; u++)
        for (int ch = 0; ch < vs.chunks; ch++)
            for (int lane = 0; lane < 64; lane++)
                for (int half = 0; half < 2; half++) {
                    const size_t site = u * PLK_V4S_UNIT + (size_t)half * 64 + lane;
                    image[plk_stream_dword(u, ch, lane, half, vs.chunks)] =
                        plk_stream_site_dword(codes.data(), Spad, site, vs.obs_row.data(), vs.nobs, rn.data(), nrows, nchar, ch);
                }
    auto need = [&](int n, size_t site) {
        unsigned v = codes[(size_t)need_b[n] * Spad + site];
        if (need_c[n] >= 0) v = v * (unsigned)nchar + codes[(size_t)need_c[n] * Spad + site];
        return v;
    };

    /* the interpreter's fetches: a wave-wide load of chunk q of unit u reads dwords [base + q * 128 + 2 lane, + 2) */
    const int cats[2] = {0, C - 1};
    for (int ci = 0; ci < (C > 1 ? 2 : 1); ci++) {
        const unsigned *wd = &vs.words[(size_t)cats[ci] * vs.stride];
        for (size_t u = 0; u < nunits; u++)
            for (int lane = 0; lane < 64; lane += (u == 0 || u + 1 == nunits) ? 1 : 21) {
                const size_t ubase = u * (size_t)vs.chunks * PLK_V4S_UNIT;
                auto load = [&](size_t q, unsigned out[2]) -> bool {
                    const size_t at = ubase + q * PLK_V4S_UNIT + 2 * (size_t)lane;
                    if (at + 2 > total) return false;
                    if (at != plk_stream_dword(u, (int)q, lane, 0, vs.chunks) || plk_stream_byte(u, (int)q, lane, 1, 3, vs.chunks) != (at + 1) * 4 + 3) return false;
                    out[0] = image.at(at); out[1] = image.at(at + 1);
                    return true;
                };
                unsigned cur[2], ring[2][2];
                size_t next_chunk = 3;
                if (!load(0, cur) || !load(1, ring[0]) || !load(2, ring[1])) return "replay: the prologue loads outside the stream";
                const size_t siteA = u * PLK_V4S_UNIT + lane, siteB = siteA + 64;
                if ((cur[0] & 0xff) != need(0, siteA) || (cur[1] & 0xff) != need(0, siteB)) return "replay: the prologue extracts the wrong code";
                int oi = 0;
                bool done = false;
                for (size_t w = 0; !done && w < vs.stride / 2; w++) {
                    const unsigned hidx = wd[2 * w] / PLK_V4_HANDLER_BYTES, hi = wd[2 * w + 1];
                    if (hidx == OP_END) { done = true; break; }
                    if (hidx == PLK_V4S_ADVANCE || hidx == PLK_V4S_ADVANCE + 1) {
                        const int k = (int)(hidx - PLK_V4S_ADVANCE);
                        cur[0] = ring[k][0]; cur[1] = ring[k][1];
                        if (!load(next_chunk++, ring[k])) return "replay: an ADVANCE loads outside the stream";
                        continue;
                    }
                    if (!plk_word_is_obs(hidx)) continue;
                    const int nx = oi + 1 < nobs ? oi + 1 : oi;
                    const unsigned a = (cur[0] >> (hi & 31)) & 0xff, b = (cur[1] >> (hi & 31)) & 0xff;
                    if (a != need(nx, siteA) || b != need(nx, siteB))
                        return "replay: observation " + std::to_string(oi) + " extracts " + std::to_string(a) + " / " + std::to_string(b) + ", the program needs " +
                               std::to_string(need(nx, siteA)) + " / " + std::to_string(need(nx, siteB));
                    oi++;
                    g_obs++;
                }
                if (!done || oi != nobs) return "replay: the op stream ends after " + std::to_string(oi) + " of " + std::to_string(nobs) + " observations";
            }
    }

    /* negative controls */
    {
        PlkFusedV4S v2 = vs;
        const size_t c0 = (size_t)(C - 1) * vs.stride;
        size_t obs_at = (size_t)-1, adv_at = (size_t)-1;
        for (size_t w = 0; w < vs.stride / 2; w++) {
            const unsigned hidx = vs.words[c0 + 2 * w] / PLK_V4_HANDLER_BYTES;
            if (obs_at == (size_t)-1 && hidx < 32 && plk_word_is_obs(hidx)) obs_at = c0 + 2 * w;
            if (adv_at == (size_t)-1 && (hidx == PLK_V4S_ADVANCE || hidx == PLK_V4S_ADVANCE + 1)) adv_at = c0 + 2 * w;
        }
        if (obs_at == (size_t)-1) return "no observation op in the stream";
        v2.words[obs_at + 1] ^= 8u;
        if (plk_fused_check_v4s(fp, v2, nchar, C, tip_base, lds).empty()) return "negative control: wrong byte position accepted";
        v2 = vs;
        v2.words[obs_at + 1] = (v2.words[obs_at + 1] & 0xffffu) | ((unsigned)((tip_base + lds) / 32) << 16);
        if (plk_fused_check_v4s(fp, v2, nchar, C, tip_base, lds).empty()) return "negative control: table field past the image accepted";
        v2 = vs;
        v2.chunks--;
        if (plk_fused_check_v4s(fp, v2, nchar, C, tip_base, lds).empty()) return "negative control: missing spare chunk accepted";
        if (adv_at != (size_t)-1) {
            v2 = vs;
            v2.words[adv_at] ^= (unsigned)PLK_V4_HANDLER_BYTES;      /* ADVANCE_0 <-> ADVANCE_1 */
            if (plk_fused_check_v4s(fp, v2, nchar, C, tip_base, lds).empty()) return "negative control: ADVANCE of the wrong kind accepted";
            v2 = vs;
            v2.words[adv_at] = OP_SCALE * PLK_V4_HANDLER_BYTES;        /* a lost ADVANCE */
            if (plk_fused_check_v4s(fp, v2, nchar, C, tip_base, lds).empty()) return "negative control: lost ADVANCE accepted";
        }
        v2 = vs;
        if (nobs > 1) {
            std::swap(v2.obs_row[0], v2.obs_row[1]);
            if (v2.obs_row != vs.obs_row && plk_fused_check_v4s(fp, v2, nchar, C, tip_base, lds).empty()) return "negative control: swapped stream rows accepted";
        }
        if (plk_fused_check_v4s(fp, vs, nchar, C, tip_base, lds - 32).empty()) return "negative control: short LDS accepted";
    }
    return "";
}

int main()
{
    std::mt19937_64 rng(20250355), crng(777);
    auto rnd = [&](int n) { return (int)(rng() % (unsigned long long)n); };
    const int nchars[3] = {4, 5, 16}, Cs[2] = {1, 4};
    const long Ss[3] = {1, 129, 300};
    for (int iter = 0; iter < 6000; iter++) {
        const int shape = iter % 8;
        int N;
        if (shape == 7) N = 2 + rnd(3);
        else if (iter % 97 == 0) N = 500 + rnd(3000);
        else N = 2 + rnd(iter % 5 == 0 ? 300 : 40);
        std::vector<int> ea(N - 1), eb(N - 1), label(N);
        for (int i = 0; i < N; i++) label[i] = i;
        for (int i = N - 1; i > 0; i--) std::swap(label[i], label[rnd(i + 1)]);
        for (int i = 1; i < N; i++) {
            int parent;
            switch (shape) {
            case 0: parent = rnd(i); break;
            case 1: parent = i - 1; break;
            case 2: parent = (i - 1) / 2; break;
            case 3: parent = i % 2 ? i - 1 - (i > 1) : i - 2; if (parent < 0) parent = 0; break;
            case 4: parent = 0; break;
            case 5: parent = rnd(10) < 7 ? rnd(i) : std::max(0, i - 1 - rnd(std::min(i, 3))); break;
            case 6: parent = (i - 1) / 3; break;
            default: parent = rnd(i); break;
            }
            ea[i - 1] = label[parent]; eb[i - 1] = label[i];
        }
        for (int e = N - 2; e > 0; e--) { const int j = rnd(e + 1); std::swap(ea[e], ea[j]); std::swap(eb[e], eb[j]); }
        Tree t;
        if (!make_tree(N, ea, eb, t)) { fprintf(stderr, "generator produced a non-tree\n"); return 2; }
        std::vector<char> has(N, 0);
        const int pdata = iter % 3 == 0 ? 0 : (iter % 3 == 1 ? 30 : 100);
        for (int a = 0; a < N; a++) has[a] = t.ip[a + 1] > t.ip[a] && rnd(100) < pdata;
        (void)rnd(8);                         /* progcheck draws its nchar here: keep the tree sequence the same */
        const int nchar = nchars[(iter / 3) % 3], C = Cs[(iter / 9) % 2];
        const long S = Ss[(iter / 18) % 3];
        const std::string bad = check_tree(t, has, nchar, C, S, crng);
        if (!bad.empty()) { fprintf(stderr, "iteration %d (shape %d, N = %d, nchar = %d, C = %d, S = %ld): %s\n", iter, shape, N, nchar, C, S, bad.c_str()); return 1; }
    }
    printf("ok %ld %ld\n", g_taken, g_obs);
    return 0;
}
