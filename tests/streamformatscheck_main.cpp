/*
 * tests/streamformatscheck_main.cpp -- CPU driver for the sequence that derives the formats the streamed k = 4 kernel runs
 * (plk_k4_stream in phyly_amd/csrc/plk_program.h: tables and category groups, the folded and the pair-product stream, the
 * fall-backs between them, the barrier), built with AddressSanitizer + UBSan by tests/test_k4_stream_formats_host.py.
 *
 * Trees, the smallest that reach each branch: 3 leaves (no absorbed node), the 4-leaf caterpillar (one three-leaf table), the
 * 5-leaf shapes of tests/test_gpu_k4_triple.py, the 39-leaf 4-slot tree of tests/test_gpu_k4_fold.py (no pair products), the
 * 40-leaf caterpillar (rescaling, a stand-alone SCALE) and, from the file given as argument, the tree of BASELINE config 3
 * (four-leaf tables, a group per category).  Every leaf is given the four codes of fully observed data.  Per tree: the nchar of
 * {4, 5, 6, 16} and the C of {1, 3, 4} whose tables fit the LDS (listed below, not found out: a case that is not a checked
 * streamed choice fails the run), S in {1, 129, 300, 1 250 000, 10 000 000}, 256 CUs and 1, twelve values of
 * PLK_OPT_PAIR_TABLES, and the 16 combinations of the four capabilities (the large trees: all on, each one off, all off and
 * one more that rotates with the case).  For every case:
 *   (a) what the result names as running replays when checked again here: plk_fused_check_v4s with the returned LDS and
 *       resident categories, plk_fused_check_v4s_fold, plk_fused_check_v4p, plk_fused_check_v4t / _v4q against the checked program;
 *   (b) what the launch relies on: groups > 1 only with pair products and room for the partial sums; pair products only with
 *       the fold and held chunks; held chunks only with the capability; no more chunks than the checked stream; the stride is
 *       that of the words named; the info words decode to the plan and the fold's counters; the barrier is plk_v4s_auto_sync
 *       of what runs unless an option bit forces it;
 *   (c) a capability off gives what the option bit gives: held off = + 128, pair off = + 512 (compared by the hash below);
 *       groups off or no room: one group with the table count of plk_v4t_plan(..., groups_opt = 1);
 *   (d) six outcomes are counted and each must occur: the checked, the folded, the pair-product words run; tables in one group,
 *       in more than one; tables of the choice's plan taken back (the groups, for want of a capability).
 * With all capabilities on, a 64-bit FNV-1a hash per tree over the cases in order -- the words that run, the table, row and
 * matrix lists of the pair-table format that runs, obs_row, chunks, first_y, the LDS, sync and the four info words -- is
 * printed as "hash <tree> <hex>" for the test to compare.
 * Prints "ok <cases> <outcome counts>" and exits 0, or the first failure and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plk_program.h"

struct Tree { std::string name; int N; std::vector<int> ip, ix, pre; std::vector<int> nchars, Cs; bool large; };

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

/* nested brackets, 0 = a leaf, as _shape_edges of tests/test_gpu_k4_fold.py: leaves numbered in order of appearance, internal nodes after them */
static int walk(const char *&s, int &leaf, int &inner, std::vector<int> &ea, std::vector<int> &eb)
{
    if (*s == '0') { s++; return leaf++; }
    std::vector<int> kids;
    for (s++; *s != ')'; ) { kids.push_back(walk(s, leaf, inner, ea, eb)); if (*s == ',') s++; }
    s++;
    const int me = inner++;
    for (int k : kids) { ea.push_back(me); eb.push_back(k); }
    return me;
}
static bool shaped_tree(const std::string &shape, Tree &t)
{
    int leaf = 0, inner = 0;
    for (char c : shape) inner += c == '0';
    std::vector<int> ea, eb;
    const char *s = shape.c_str();
    walk(s, leaf, inner, ea, eb);
    return make_tree(inner, ea, eb, t);
}
static std::string cat(int n) { std::string s = "(0,0)"; for (int i = 2; i < n; i++) s = "(" + s + ",0)"; return s; }
static std::string bal(int n) { return n == 1 ? "0" : "(" + bal(n - n / 2) + "," + bal(n / 2) + ")"; }

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
template <typename T> static uint64_t fnv_vec(uint64_t h, const std::vector<T> &v) { const uint64_t n = v.size(); h = fnv(h, &n, 8); return v.empty() ? h : fnv(h, v.data(), v.size() * sizeof(T)); }
static uint64_t fnv_long(uint64_t h, long v) { const int64_t x = v; return fnv(h, &x, 8); }

static uint64_t hash_result(uint64_t h, const PlkK4Stream &r, const PlkFusedPT &f)
{
    h = fnv_vec(h, r.words());
    h = fnv_vec(h, f.tab_unit); h = fnv_vec(h, f.tab_edge); h = fnv_vec(h, f.tab_eb); h = fnv_vec(h, f.tab_ec); h = fnv_vec(h, f.tab_ea); h = fnv_vec(h, f.tab_el);
    h = fnv_vec(h, f.tab_shape); h = fnv_vec(h, f.tab_et); h = fnv_vec(h, f.tab_ef); h = fnv_vec(h, f.tab_eg); h = fnv_vec(h, f.tab_row);
    h = fnv_vec(h, f.row_node); h = fnv_vec(h, f.row_node2); h = fnv_vec(h, f.row_node3); h = fnv_vec(h, f.row_node4); h = fnv_vec(h, f.mat_edge);
    h = fnv_vec(h, r.fv4s.obs_row); h = fnv_long(h, r.fv4s.chunks); h = fnv_vec(h, r.fv4s.first_y);
    h = fnv_long(h, (long)r.lds); h = fnv_long(h, r.sync);
    h = fnv_long(h, r.info_fold); h = fnv_long(h, r.info_pairmul); h = fnv_long(h, r.info_triple); h = fnv_long(h, r.info_quad);
    return h;
}

enum { OUT_CHECKED, OUT_FOLDED, OUT_PAIR, OUT_ONE_GROUP, OUT_GROUPS, OUT_TAKEN_BACK, OUT_COUNT };
static long g_outcome[OUT_COUNT], g_cases;

struct Run { PlkK4Stream r; PlkFusedPT fpt; };

/* one case: the choice of the shape, then the sequence under `caps` */
static std::string run_case(const Tree &t, const PlkProgram &pg, PlkK4Shape sh, const PlkK4StreamCaps &caps, Run &out, PlkK4Choice *chosen = nullptr, PlkFusedPT *checked = nullptr,
                            PlkFusedV4S *checked_stream = nullptr)
{
    PlkFused fu; PlkFusedV4 fv4; PlkFusedV4S fv4s;
    const PlkK4Choice ch = plk_k4_choose(t.N, t.ip.data(), t.ix.data(), pg, sh, true, fu, out.fpt, fv4, fv4s);
    if (ch.variant != PLK_K4_V4S || !ch.bad.empty()) return "the list holds a case that is no checked streamed choice (" + ch.bad + ")";
    if (chosen) *chosen = ch;
    if (checked) *checked = out.fpt;
    if (checked_stream) *checked_stream = fv4s;
    out.r = plk_k4_stream(t.N, t.ip.data(), t.ix.data(), pg, sh, ch, caps, out.fpt, std::move(fv4s));
    return "";
}

static std::string check_case(const Tree &t, const PlkProgram &pg, const PlkK4Shape &sh, const PlkK4StreamCaps &caps, uint64_t *hash)
{
    const int nchar = sh.nchar, C = sh.C;
    Run run;
    PlkK4Choice ch;
    PlkFusedPT in;
    PlkFusedV4S vin;
    std::string bad = run_case(t, pg, sh, caps, run, &ch, &in, &vin);
    if (!bad.empty()) return bad;
    const PlkK4Stream &r = run.r;
    const PlkFusedPT &f = run.fpt;
    const PlkPairTablesOpt po = plk_pair_tables_opt(sh.pair_tables);
    const bool tables = r.triple.nodes + r.triple.quads > 0;
    if (!r.note.empty()) return "a derived form was not taken: " + r.note;
    g_cases++;

    /* (a) */
    const int Cg = r.Cg(C);
    if (r.fv4s.Cg != Cg) return "the stream that runs is laid out for other resident categories than the plan's";
    if (r.lds != plk_fused_v4s_lds_bytes(f, nchar, Cg)) return "the LDS is not that of the format that runs";
    if (!(bad = plk_fused_check_v4s(f, r.fv4s, nchar, C, ch.tip_base, r.lds)).empty()) return bad;
    if (r.runs != PlkK4Stream::CHECKED && !(bad = plk_fused_check_v4s_fold(r.fv4s, r.fold)).empty()) return bad;
    if (r.runs == PlkK4Stream::PAIR && !(bad = plk_fused_check_v4p(r.fv4s, r.pair)).empty()) return bad;
    if (tables) {
        bad = r.triple.quads > 0 ? plk_fused_check_v4q(t.N, t.ip.data(), t.ix.data(), in, f, nchar, sh.node_codes) : plk_fused_check_v4t(t.N, t.ip.data(), t.ix.data(), in, f, nchar);
        if (!bad.empty()) return bad;
        if (f.ntriples != r.triple.nodes || f.nquads != r.triple.quads) return "the format that runs holds other tables than the plan";
    } else if (f.words != in.words || f.mat_edge != in.mat_edge || f.units != in.units || r.fv4s.words != vin.words || r.lds != ch.lds) return "no tables, but not the checked formats";

    /* (b) */
    if (r.triple.groups > 1 && (r.runs != PlkK4Stream::PAIR || !caps.partial_sums || !caps.groups || !tables)) return "category groups without what the launch needs";
    if (r.runs == PlkK4Stream::PAIR && (!r.held || !ch.fold || !caps.pair || !ch.pair)) return "pair products without the fold, the held chunks or the capability";
    if (r.runs != PlkK4Stream::CHECKED && !ch.fold) return "a fold that was not asked for";
    if (r.held && (!caps.held || !ch.held)) return "held chunks without the capability";
    if (r.fv4s.chunks > vin.chunks) return "more chunks than the checked stream";
    if (r.words().size() != (size_t)C * r.stride() || &r.words() != (r.runs == PlkK4Stream::PAIR ? &r.pair.words : r.runs == PlkK4Stream::FOLDED ? &r.fold.words : &r.fv4s.words))
        return "the stride is not that of the words named";
    const long want_triple = tables ? 1 | (long)r.triple.groups << 4 | (long)r.triple.nodes << 8 : 0, want_quad = r.triple.quads > 0 ? 1 | (long)r.triple.quads << 8 : 0;
    if (r.triple.groups > 15 || r.info_triple != want_triple || r.info_quad != want_quad) return "PLK_INFO_LL_TRIPLE / _QUAD do not decode to the plan";
    const PlkFusedV4SFold &fo = r.fold;
    const long want_fold = (r.held ? 2 : 0) | (r.runs == PlkK4Stream::CHECKED ? 0 : 1 | (long)(fo.scale_slots & 15) << 4 | (long)std::min(fo.standalone_scale, 255) << 8 |
                                                                                       (long)std::min(fo.nadv[0], 255) << 16 | (long)std::min(fo.nadv[1], 127) << 24);
    if (r.info_fold != want_fold) return "PLK_INFO_LL_FOLD does not decode to the fold's counters";
    if (r.info_pairmul != (r.runs == PlkK4Stream::PAIR ? 1 | (long)std::min(r.pair.npair, 65535) << 8 : 0)) return "PLK_INFO_LL_PAIRMUL";
    if (r.sync_auto != (po.sync < 0) || r.sync != (po.sync < 0 ? plk_v4s_auto_sync(Cg, f.mat_edge.size(), r.words().size() / (size_t)C) : po.sync)) return "the barrier";

    /* (c) */
    const uint64_t mine = hash_result(1469598103934665603ull, r, f);
    auto same_as_bit = [&](long bit, PlkK4StreamCaps c2) -> std::string {
        PlkK4Shape s2 = sh;
        s2.pair_tables |= bit;
        Run other;
        const std::string b2 = run_case(t, pg, s2, c2, other);
        if (!b2.empty()) return b2;
        return hash_result(1469598103934665603ull, other.r, other.fpt) == mine && other.r.runs == r.runs && other.r.held == r.held && other.r.triple.groups == r.triple.groups ? "" : plk_fmt("a capability off and + %ld differ", bit);
    };
    if (!caps.held) { PlkK4StreamCaps c2 = caps; c2.held = true; if (!(bad = same_as_bit(128, c2)).empty()) return bad; }
    if (!caps.pair) { PlkK4StreamCaps c2 = caps; c2.pair = true; if (!(bad = same_as_bit(512, c2)).empty()) return bad; }
    if (!caps.groups || !caps.partial_sums) {
        const PlkV4TPlan one = plk_v4t_plan(in, nchar, C, sh.S, sh.num_cus, ch.tip_base, po.triple, 1, po.quad, sh.node_codes);
        if (r.triple.groups != 1 || r.triple.nodes != one.nodes || r.triple.quads != one.quads) return "groups off or no room: not the tables of the plan with one group";
    }

    /* (d) */
    g_outcome[r.runs == PlkK4Stream::PAIR ? OUT_PAIR : r.runs == PlkK4Stream::FOLDED ? OUT_FOLDED : OUT_CHECKED]++;
    if (tables) g_outcome[r.triple.groups > 1 ? OUT_GROUPS : OUT_ONE_GROUP]++;
    if (ch.triple.nodes + ch.triple.quads > 0 && (r.triple.groups != ch.triple.groups || r.triple.nodes != ch.triple.nodes || r.triple.quads != ch.triple.quads)) g_outcome[OUT_TAKEN_BACK]++;
    if (hash) *hash = hash_result(*hash, r, f);
    return "";
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: streamformatscheck TREE\n"); return 2; }
    std::vector<Tree> trees;
    auto add = [&](const char *name, const std::string &shape, std::vector<int> nchars, std::vector<int> Cs, bool large) {
        Tree t;
        if (!shaped_tree(shape, t)) { fprintf(stderr, "%s: not a tree\n", name); exit(2); }
        t.name = name; t.nchars = nchars; t.Cs = Cs; t.large = large;
        trees.push_back(t);
    };
    add("three", "((0,0),0)", {4, 5, 6, 16}, {1, 3, 4}, false);
    add("four", "(((0,0),0),0)", {4, 5, 6, 16}, {1, 3, 4}, false);
    add("tip_mul", "((((0,0),0),0),0)", {4, 5, 6, 16}, {1, 3, 4}, false);
    add("matvec", "(((((0,0),0),),0),0)", {4, 5, 6, 16}, {1, 3, 4}, false);
    add("push", "(((0,0),0),(0,0))", {4, 5, 6, 16}, {1, 3, 4}, false);
    add("popmul", "((0,0),((0,0),0))", {4, 5, 6, 16}, {1, 3, 4}, false);
    const std::string five = "(" + cat(5) + "," + cat(5) + ")";
    add("slots4", "(" + bal(16) + ",(" + bal(8) + ",(" + five + "," + five + ")))", {4, 5}, {1, 3, 4}, true);
    add("cat40", cat(40), {4, 5, 6}, {1, 3, 4}, true);
    {
        Tree t;
        FILE *f = fopen(argv[1], "r");
        if (!f || fscanf(f, "%d", &t.N) != 1 || t.N < 2 || t.N > 100000) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        t.ip.resize(t.N + 1); t.ix.resize(t.N - 1); t.pre.resize(t.N);
        bool ok = true;
        for (int &x : t.ip) ok = ok && fscanf(f, "%d", &x) == 1;
        for (int &x : t.ix) ok = ok && fscanf(f, "%d", &x) == 1 && x >= 0 && x < t.N;
        for (int &x : t.pre) ok = ok && fscanf(f, "%d", &x) == 1 && x >= 0 && x < t.N;
        fclose(f);
        if (!ok || t.ip[0] != 0 || t.ip[t.N] != t.N - 1) { fprintf(stderr, "%s: not a tree file\n", argv[1]); return 2; }
        t.name = "config3"; t.nchars = {4, 5}; t.Cs = {1, 3, 4}; t.large = true;
        trees.push_back(t);
    }
    const long Ss[] = {1, 129, 300, 1250000, 10000000}, opts[] = {1, 1 + 64, 1 + 128, 1 + 256, 1 + 512, 1 + 1024, 1 + 1024 + 4096, 1 + 1024 + 4096 + 8192, 1 + 1024 + 8192, 1 + 2048, 1 + 16384, 1 + 32768};
    const int cus[] = {256, 1};
    for (const Tree &t : trees) {
        std::vector<char> has(t.N, 0);
        std::vector<int> masks(t.N, 0);
        for (int a = 0; a < t.N; a++) if (t.ip[a + 1] == t.ip[a]) masks[a] = 0xf;
        PlkProgram pg;
        plk_program_build(t.N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
        uint64_t hash = 1469598103934665603ull;
        long n = 0;
        for (int nchar : t.nchars) for (int C : t.Cs) for (long S : Ss) for (int cu : cus) for (long opt : opts) {
            PlkK4Shape sh = {nchar, C, S, cu, opt, 1, 0, {4608, 0, 0}};
            sh.node_codes = masks.data();
            for (int m = 15; m >= 0; m--) {
                /* bit set: the capability is there.  Large trees: all, all but one, none, and one combination more */
                const int off = 15 - m;
                if (t.large && off != 0 && off != 15 && (off & (off - 1)) != 0 && m != (int)(n % 16)) continue;
                PlkK4StreamCaps caps;
                caps.held = m & 1; caps.pair = m & 2; caps.groups = m & 4; caps.partial_sums = m & 8;
                const std::string bad = check_case(t, pg, sh, caps, m == 15 ? &hash : nullptr);
                if (!bad.empty()) {
                    fprintf(stderr, "%s, nchar %d, C %d, S %ld, %d CUs, option %ld, capabilities %d: %s\n", t.name.c_str(), nchar, C, S, cu, opt, m, bad.c_str());
                    return 1;
                }
            }
            n++;
        }
        printf("hash %s %016llx\n", t.name.c_str(), (unsigned long long)hash);
    }
    printf("ok %ld", g_cases);
    for (int q = 0; q < OUT_COUNT; q++) printf(" %ld", g_outcome[q]);
    printf("\n");
    return 0;
}
