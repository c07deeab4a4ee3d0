/*
 * tests/foldcheck_main.cpp -- CPU driver for the FOLDED op stream of the streamed k = 4 interpreter (k_ll_fused4_v4s;
 * plk_v4s_fold_ops, plk_fused_v4s_fold and plk_fused_check_v4s_fold in phyly_amd/csrc/plk_program.h), built with
 * AddressSanitizer + UBSan by tests/test_k4_fold_host.py.
 *
 * Over the seeded random trees of tests/progcheck_main.cpp (same generator, same seed, same 6000 iterations, the skip
 * rules of tests/streamcheck_main.cpp) it builds the checked stream and its fold and requires, for every tree taken:
 *   - the replay check accepts the fold;
 *   - unfolding the folded ops and cutting them into blocks again gives the checked stream's words exactly;
 *   - no ADVANCE keeps a dispatch of its own, and a SCALE does only where the op before it is not MATVEC + POPMUL;
 *   - the END is there, two whole blocks follow its block, and they hold nothing but END and REFILL ops;
 *   - the replay check rejects: a folded ADVANCE of the other kind, a + SCALE variant where no SCALE followed, a dropped
 *     observation op, a REFILL of the other kind.
 * With a file name as argument (N, then indptr, indices, preorder of a tree without data on internal nodes; nchar 5,
 * C 4: what tests/test_k4_fold_host.py writes from synth.Workload(3)) it also requires the dispatch counts of one
 * category of BASELINE config 3: 161 = 114 + 20 REFILL + 16 ADVANCE + 10 SCALE + 1 END unfolded; folded, no ADVANCE and
 * at most 2 SCALE dispatches.
 * Prints "ok <trees taken> <ADVANCEs folded> <SCALEs folded> <SCALEs left> <controls run: kind, scale, drop, refill>"
 * and exits 0, or the first failure and exits 1.
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

static long g_taken = 0, g_adv = 0, g_scale = 0, g_scale_left = 0, g_ctl[4] = {0, 0, 0, 0};

struct Histogram { long ops = 0, refill = 0, advance = 0, scale = 0, end = 0; };

/* the dispatches of one category up to and with its END */
static Histogram histogram(const unsigned *wd, size_t stride)
{
    Histogram hg;
    for (size_t i = 0; i < stride / 2; i++) {
        const unsigned h = wd[2 * i] / PLK_V4_HANDLER_BYTES;
        if (h == OP_END) { hg.end++; break; }
        if (h == (unsigned)PLK_V4_REFILL_A || h == (unsigned)PLK_V4_REFILL_B) hg.refill++;
        else if (h == (unsigned)PLK_V4S_ADVANCE || h == (unsigned)PLK_V4S_ADVANCE + 1) hg.advance++;
        else if (h == OP_SCALE) hg.scale++;
        else hg.ops++;
    }
    return hg;
}

static bool is_advance(unsigned h) { return h == (unsigned)PLK_V4S_ADVANCE || h == (unsigned)PLK_V4S_ADVANCE + 1; }
static bool is_fold_adv(unsigned h) { return h >= PLK_V4S_FOLD_ADV && h < PLK_V4S_FOLD_SCALE; }
static bool is_fold_scale(unsigned h) { return h >= PLK_V4S_FOLD_SCALE && h < PLK_V4S_FOLD_SCALE + 4; }

/* a fold whose category streams are `ops` cut into blocks (every category the same list: enough for a control) */
static PlkFusedV4SFold reblocked(const PlkFusedV4S &vs, const std::vector<std::vector<PlkV4SOp>> &ops)
{
    PlkFusedV4SFold fo;
    fo.stride = plk_v4s_block_stride(ops[0].size());
    fo.words.assign((size_t)vs.C * fo.stride, 0u);
    for (int c = 0; c < vs.C; c++) plk_v4s_block_ops(ops[c], &fo.words[(size_t)c * fo.stride], fo.stride);
    return fo;
}

static std::string check_tree(const Tree &t, const std::vector<char> &has, int nchar, int C, Histogram *unfolded, Histogram *folded_out)
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

    PlkFusedV4SFold fo;
    plk_fused_v4s_fold(vs, fo);
    bad = plk_fused_check_v4s_fold(vs, fo);
    if (!bad.empty()) return bad;
    if (fo.stride > vs.stride) return "the folded stream is longer than the checked one";
    if (unfolded) *unfolded = histogram(vs.words.data(), vs.stride);
    if (folded_out) *folded_out = histogram(fo.words.data(), fo.stride);

    std::vector<std::vector<PlkV4SOp>> fops(C);
    for (int c = 0; c < C; c++) {
        const unsigned *wd = &fo.words[(size_t)c * fo.stride];
        std::vector<PlkV4SOp> src, un;
        if (!plk_v4s_stream_ops(wd, fo.stride, fops[c])) return "the folded stream has no END";
        if (!plk_v4s_stream_ops(&vs.words[(size_t)c * vs.stride], vs.stride, src)) return "the checked stream has no END";
        /* unfolded and cut into blocks again: the checked stream's words */
        plk_v4s_unfold_ops(fops[c], un);
        if (plk_v4s_block_stride(un.size()) != vs.stride) return "unfolding gives another stride than the checked stream's";
        std::vector<unsigned> back(vs.stride);
        plk_v4s_block_ops(un, back.data(), vs.stride);
        for (size_t i = 0; i < vs.stride; i++) if (back[i] != vs.words[(size_t)c * vs.stride + i]) return "unfolding does not give the checked stream's word " + std::to_string(i);
        /* what keeps a dispatch of its own */
        long nadv_src = 0, nscale_src = 0, nadv = 0, nscale = 0, left = 0;
        for (const PlkV4SOp &op : src) { nadv_src += is_advance(op.h); nscale_src += op.h == OP_SCALE; }
        for (size_t i = 0; i < fops[c].size(); i++) {
            const unsigned h = fops[c][i].h;
            if (is_advance(h)) return "an ADVANCE keeps its own dispatch";
            if (h == OP_SCALE) {
                if (i > 0 && fops[c][i - 1].h >= 28 && fops[c][i - 1].h < 32) return "a SCALE after MATVEC + POPMUL keeps its own dispatch";
                left++;
            }
            nadv += is_fold_adv(h); nscale += is_fold_scale(h);
        }
        if (nadv != nadv_src || nscale + left != nscale_src) return "folded and left ops do not add up to the checked stream's";
        if (src.size() != fops[c].size() + (size_t)nadv + (size_t)nscale) return "the fold removed other ops than ADVANCE and SCALE";
        if (c == 0) {
            g_adv += nadv; g_scale += nscale; g_scale_left += left;
            if (fo.nadv[0] + fo.nadv[1] != nadv || fo.standalone_scale != left || fo.standalone_adv != 0) return "the fold's counts";
            unsigned slots = 0;
            for (const PlkV4SOp &op : fops[c]) if (is_fold_scale(op.h)) slots |= 1u << (op.h - PLK_V4S_FOLD_SCALE);
            if (slots != fo.scale_slots) return "the fold's + SCALE slots";
        }
        /* END, then nothing but END and REFILL, two whole blocks after the END's block */
        size_t end_at = (size_t)-1;
        for (size_t i = 0; i < fo.stride / 2 && end_at == (size_t)-1; i++) if (wd[2 * i] == (unsigned)OP_END * PLK_V4_HANDLER_BYTES) end_at = i;
        if (end_at == (size_t)-1) return "no END";
        if (end_at / 8 + 3 != fo.stride / 16) return "not exactly two spare blocks after the END's block";
        for (size_t i = end_at; i < fo.stride / 2; i++) {
            const unsigned want = i % 8 == 7 ? (unsigned)(((i / 8) & 1) ? PLK_V4_REFILL_B : PLK_V4_REFILL_A) : (unsigned)OP_END;
            if (wd[2 * i] != want * PLK_V4_HANDLER_BYTES || wd[2 * i + 1] != 0) return "the spare blocks hold another op than END and REFILL";
        }
    }

    /* negative controls */
    {
        std::vector<std::vector<PlkV4SOp>> m = fops;
        size_t at = (size_t)-1;
        for (size_t i = 0; i < m[C - 1].size() && at == (size_t)-1; i++) if (is_fold_adv(m[C - 1][i].h)) at = i;
        if (at != (size_t)-1) {
            m[C - 1][at].h ^= 1u;
            if (plk_fused_check_v4s_fold(vs, reblocked(vs, m)).empty()) return "negative control: folded ADVANCE of the wrong kind accepted";
            g_ctl[0]++;
        }
        m = fops; at = (size_t)-1;
        for (size_t i = 0; i < m[0].size() && at == (size_t)-1; i++) if (m[0][i].h >= 28 && m[0][i].h < 32) at = i;
        if (at != (size_t)-1) {
            m[0][at].h += PLK_V4S_FOLD_SCALE - 28;
            if (plk_fused_check_v4s_fold(vs, reblocked(vs, m)).empty()) return "negative control: + SCALE variant without a SCALE accepted";
            g_ctl[1]++;
        }
        m = fops; at = (size_t)-1;
        for (size_t i = 0; i < m[0].size() && at == (size_t)-1; i++) if (plk_v4s_obs_index(m[0][i].h) >= 0 || is_fold_adv(m[0][i].h)) at = i;
        if (at == (size_t)-1) return "no observation op in the folded stream";
        for (int c = 0; c < C; c++) m[c].erase(m[c].begin() + (long)at);
        if (plk_fused_check_v4s_fold(vs, reblocked(vs, m)).empty()) return "negative control: dropped observation op accepted";
        g_ctl[2]++;
        PlkFusedV4SFold f2 = fo;
        f2.words[(size_t)(C - 1) * fo.stride + 2 * 7] ^= (unsigned)PLK_V4_HANDLER_BYTES;       /* REFILL_A <-> REFILL_B */
        if (plk_fused_check_v4s_fold(vs, f2).empty()) return "negative control: REFILL of the wrong kind accepted";
        g_ctl[3]++;
    }
    return "";
}

static int config3(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    Tree t;
    bool ok = fscanf(f, "%d", &t.N) == 1 && t.N >= 2 && t.N < 100000;
    if (ok) {
        t.ip.resize(t.N + 1); t.ix.resize(t.N - 1); t.pre.resize(t.N);
        for (int &v : t.ip) ok = ok && fscanf(f, "%d", &v) == 1;
        for (int &v : t.ix) ok = ok && fscanf(f, "%d", &v) == 1 && v >= 0 && v < t.N;
        for (int &v : t.pre) ok = ok && fscanf(f, "%d", &v) == 1 && v >= 0 && v < t.N;
        ok = ok && t.ip[0] == 0 && t.ip[t.N] == t.N - 1;
        for (int a = 0; ok && a < t.N; a++) ok = t.ip[a + 1] >= t.ip[a];
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: not a tree file\n", path); return 2; }
    const long before = g_taken;
    Histogram u, fo;
    const std::string bad = check_tree(t, std::vector<char>(t.N, 0), 5, 4, &u, &fo);
    if (!bad.empty() || g_taken == before) { fprintf(stderr, "config 3 tree: %s\n", bad.empty() ? "not taken by the streamed form" : bad.c_str()); return 1; }
    if (u.ops != 114 || u.refill != 20 || u.advance != 16 || u.scale != 10 || u.end != 1) {
        fprintf(stderr, "config 3 tree, unfolded: %ld ops, %ld REFILL, %ld ADVANCE, %ld SCALE, %ld END (114 + 20 + 16 + 10 + 1 expected)\n", u.ops, u.refill, u.advance, u.scale, u.end);
        return 1;
    }
    if (fo.advance != 0 || fo.scale > 2 || fo.end != 1 || fo.ops != 114) {
        fprintf(stderr, "config 3 tree, folded: %ld ops, %ld REFILL, %ld ADVANCE, %ld SCALE, %ld END\n", fo.ops, fo.refill, fo.advance, fo.scale, fo.end);
        return 1;
    }
    printf("config3 %ld %ld\n", u.ops + u.refill + u.advance + u.scale + u.end, fo.ops + fo.refill + fo.advance + fo.scale + fo.end);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1) { const int rc = config3(argv[1]); if (rc) return rc; }
    std::mt19937_64 rng(20250355);
    auto rnd = [&](int n) { return (int)(rng() % (unsigned long long)n); };
    const int nchars[3] = {4, 5, 16}, Cs[2] = {1, 4};
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
        const std::string bad = check_tree(t, has, nchar, C, nullptr, nullptr);
        if (!bad.empty()) { fprintf(stderr, "iteration %d (shape %d, N = %d, nchar = %d, C = %d): %s\n", iter, shape, N, nchar, C, bad.c_str()); return 1; }
    }
    printf("ok %ld %ld %ld %ld %ld %ld %ld %ld\n", g_taken, g_adv, g_scale, g_scale_left, g_ctl[0], g_ctl[1], g_ctl[2], g_ctl[3]);
    return 0;
}
