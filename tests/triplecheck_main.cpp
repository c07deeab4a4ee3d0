/*
 * tests/triplecheck_main.cpp -- CPU driver for the THREE-LEAF TABLES of the streamed k = 4 interpreter (plk_v4t_candidates,
 * plk_fused_v4t_build, plk_fused_check_v4t, plk_v4t_row, plk_v4t_plan and the three-node rows of plk_stream_site_dword in
 * phyly_amd/csrc/plk_program.h), built with AddressSanitizer + UBSan by tests/test_k4_triple_host.py.
 *
 * Trees: caterpillars and balanced trees of 3 .. 12 leaves and a 40-leaf caterpillar (which the program rescales), each with
 * the children of every node in both orders; nchar 4, 5, 6 (the form applies) and 7, 16 (nchar^3 > 256: it must not);
 * C = 1 .. 4 with the categories in 1, 2 and C groups; LDS bounds from nothing to everything.  For every case:
 *   - the rewritten formats replay (plk_fused_check_v4t against the checked pair-table program, plk_fused_check_v4s on their
 *     streamed words, the fold and, within 3 stack slots, the pair-product derivation with their own checks);
 *   - the number of three-leaf tables is min(candidates, bound / plk_v4t_extra_bytes), taken in program order;
 *   - no table stands for the root; the SCALE ops sit where they sat (counted in ops of the checked program);
 *   - the matrix stream shrinks by exactly the absorbed nodes, and the observations and chunks with them;
 *   - VALUES: with random fp64 matrices, tables of both formats built on the host (a three-leaf row by plk_v4t_row, the
 *     function the device builder calls, from the rounded pair row, the rounded tip row and the stream's matrix) and random
 *     codes read back through plk_stream_site_dword, a host interpreter of the handlers' fp64 sequences gives the root
 *     vector of the rewritten program bit for bit as the checked program's.
 * Six deliberately wrong builders must each fail: a table indexed with the wrong code radix (fails the value replay), an
 * absorbed matrix left in the stream, a dropped SCALE, the root's cherry and leaf absorbed, the two leaves of the cherry
 * swapped in the row only, a row built from the next edge's matrix (each refused by plk_fused_check_v4t).
 * With a file name as argument (the tree of BASELINE config 3 as tests/foldcheck_main.cpp reads it; nchar 5, C 4) it prints
 * "config3 <candidates> <units> <matrices> <nodes G=1> <nodes G=2> <nodes G=C> <matrices G=2> <default groups at 10M sites>
 * <default nodes at 10M sites> <default nodes at 300 sites>" from plk_v4t_plan for the test to set against the byte budget.
 * Prints "ok <cases> <three-leaf tables> <cases without one> <controls: radix matrix scale root swap edge>" and exits 0, or
 * the first failure and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

/* a binary tree over `leaves` leaves: caterpillar (one leaf split off at every node) or balanced; flip: second child first */
static int grow(int leaves, bool balanced, bool flip, int &next, std::vector<int> &ea, std::vector<int> &eb)
{
    const int me = next++;
    if (leaves == 1) return me;
    const int left = balanced ? leaves / 2 : 1;
    std::vector<int> pa, pb;
    const int a = grow(left, balanced, flip, next, pa, pb), b = grow(leaves - left, balanced, flip, next, pa, pb);
    if (flip) { ea.push_back(me); eb.push_back(b); ea.push_back(me); eb.push_back(a); }
    else { ea.push_back(me); eb.push_back(a); ea.push_back(me); eb.push_back(b); }
    ea.insert(ea.end(), pa.begin(), pa.end()); eb.insert(eb.end(), pb.begin(), pb.end());
    return me;
}

static bool shaped_tree(int leaves, bool balanced, bool flip, Tree &t)
{
    std::vector<int> ea, eb;
    int next = 0;
    grow(leaves, balanced, flip, next, ea, eb);
    return make_tree(next, ea, eb, t);
}

static long g_cases = 0, g_tables = 0, g_none = 0, g_ctl[6] = {0, 0, 0, 0, 0, 0};

/* ---- values: host tables and a host interpreter of the handlers' fp64 sequences ---- */
struct Values {
    int nchar, E;
    std::vector<double> M;        /* [E][16], stream layout M[4 j + i] = P[i][j] */
    std::vector<double> defs;     /* [nchar][4] */
};

static void single_row(const Values &v, int e, int code, double *out)
{
    const double *d = &v.defs[(size_t)code * 4];
    if (e < 0) { for (int i = 0; i < 4; i++) out[i] = d[i]; return; }
    const double *m = &v.M[(size_t)e * 16];
    for (int i = 0; i < 4; i++) { double acc = 0.0; for (int j = 0; j < 4; j++) acc += m[4 * j + i] * d[j]; out[i] = acc; }
}
static void pair_row(const Values &v, int ea, int eb, int ec, int cb, int cc, double *out)
{
    double b[4], c[4], x[4];
    single_row(v, eb, cb, b); single_row(v, ec, cc, c);
    for (int j = 0; j < 4; j++) x[j] = b[j] * c[j];
    const double *m = &v.M[(size_t)ea * 16];
    for (int i = 0; i < 4; i++) { double acc = 0.0; for (int j = 0; j < 4; j++) acc += m[4 * j + i] * x[j]; out[i] = acc; }
}

/* radix_bug: the three-leaf rows are laid out as if the code were (code_b * nchar + code_l) * nchar + code_c */
static std::vector<double> build_tables(const PlkFusedPT &f, const Values &v, bool radix_bug = false)
{
    const int n = v.nchar;
    std::vector<double> tab((size_t)f.units * n * 4, 0.0);
    for (size_t t = 0; t < f.tab_unit.size(); t++) {
        double *out = &tab[(size_t)f.tab_unit[t] * n * 4];
        const bool tri = t < f.tab_el.size() && f.tab_el[t] >= 0;
        if (tri) {
            for (int cb = 0; cb < n; cb++) for (int cc = 0; cc < n; cc++) for (int cl = 0; cl < n; cl++) {
                double p[4], l[4];
                pair_row(v, f.tab_ea[t], f.tab_eb[t], f.tab_ec[t], cb, cc, p);
                single_row(v, f.tab_el[t], cl, l);
                const int code = radix_bug ? (cb * n + cl) * n + cc : (cb * n + cc) * n + cl;
                plk_v4t_row(&v.M[(size_t)f.tab_edge[t] * 16], p, l, out + (size_t)code * 4);
            }
        } else if (f.tab_eb[t] >= 0) {
            for (int cb = 0; cb < n; cb++) for (int cc = 0; cc < n; cc++) pair_row(v, f.tab_edge[t], f.tab_eb[t], f.tab_ec[t], cb, cc, out + (size_t)(cb * n + cc) * 4);
        } else for (int code = 0; code < n; code++) single_row(v, f.tab_edge[t], code, out + (size_t)code * 4);
    }
    return tab;
}

/* the root vector of one site: look-ups through the code stream's bytes, MATVEC as tools/gen_fused4_v4.py emits it */
static bool run_site(const PlkFusedPT &f, const Values &v, const std::vector<double> &tab, const std::vector<uint8_t> &codes, size_t Spad, size_t site, double *root)
{
    const int n = v.nchar, nrows = (int)f.row_node.size();
    std::vector<int> obs_row, rn(3 * (size_t)nrows, -1);
    for (const PlkFusedPT::VOp &o : f.vops) if (o.code == OP_TIP_SET || o.code == OP_TIP_MUL) obs_row.push_back(o.row);
    for (int r = 0; r < nrows; r++) {
        rn[r] = f.row_node[r]; rn[nrows + r] = f.row_node2[r];
        if ((size_t)r < f.row_node3.size()) rn[2 * (size_t)nrows + r] = f.row_node3[r];
    }
    double cur[4] = {0, 0, 0, 0}, slot[4][4];
    int oi = 0;
    size_t mi = 0;
    for (const PlkFusedPT::VOp &o : f.vops) {
        if (o.code == OP_TIP_SET || o.code == OP_TIP_MUL) {
            const unsigned d = plk_stream_site_dword(codes.data(), Spad, site, obs_row.data(), (int)obs_row.size(), rn.data(), nrows, n, oi / 4, 3);
            const unsigned code = (d >> (8 * (oi % 4))) & 0xffu;
            oi++;
            if ((size_t)(o.unit * n + (int)code + 1) * 4 > tab.size()) return false;
            const double *r = &tab[((size_t)o.unit * n + code) * 4];
            for (int i = 0; i < 4; i++) cur[i] = o.code == OP_TIP_SET ? r[i] : cur[i] * r[i];
        } else if (o.code == OP_MATVEC) {
            if (mi >= f.mat_edge.size() || f.mat_edge[mi] != o.edge) return false;
            const double *m = &v.M[(size_t)f.mat_edge[mi++] * 16];
            double t[4];
            for (int i = 0; i < 4; i++) { double acc = m[i] * cur[0]; for (int j = 1; j < 4; j++) acc = fma(m[4 * j + i], cur[j], acc); t[i] = acc; }
            memcpy(cur, t, sizeof t);
        } else if (o.code == OP_PUSH) memcpy(slot[o.d], cur, sizeof cur);
        else if (o.code == OP_POPMUL) { for (int i = 0; i < 4; i++) cur[i] *= slot[o.d][i]; }
        /* OP_SCALE: a power of two on both sides */
    }
    memcpy(root, cur, sizeof cur);
    return true;
}

static bool same_values(const PlkFusedPT &in, const PlkFusedPT &out, const Values &v, const std::vector<double> &tin, const std::vector<double> &tout,
                        const std::vector<uint8_t> &codes, size_t Spad, size_t S)
{
    for (size_t s = 0; s < S; s++) {
        double a[4], b[4];
        if (!run_site(in, v, tin, codes, Spad, s, a) || !run_site(out, v, tout, codes, Spad, s, b)) return false;
        if (memcmp(a, b, sizeof a) != 0) return false;
    }
    return true;
}

/* positions of the SCALE ops, counted in ops of the checked program */
static std::vector<long> scale_positions(const PlkFusedPT &f)
{
    std::vector<long> at;
    long n = 0;
    std::vector<char> tri(std::max(f.units, 1), 0);
    for (size_t t = 0; t < f.tab_unit.size(); t++) if (t < f.tab_el.size() && f.tab_el[t] >= 0) tri[f.tab_unit[t]] = 1;
    for (const PlkFusedPT::VOp &o : f.vops) {
        if (o.code == OP_SCALE) at.push_back(n);
        n += ((o.code == OP_TIP_SET || o.code == OP_TIP_MUL) && tri[o.unit]) ? 3 : 1;
    }
    return at;
}

static std::string check_tree(const Tree &t, int nchar, std::mt19937 &rng, bool controls)
{
    const int N = t.N;
    std::vector<char> has(N, 0);
    PlkProgram pg;
    plk_program_build(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
    std::string bad = plk_program_check(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
    if (!bad.empty()) return bad;
    if (pg.slots_needed > 4) return "";
    PlkFusedPT in;
    plk_fused_pt_build(N, t.ip.data(), t.ix.data(), pg, nchar, 1 << 30, in, true);
    bad = plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, in, nchar, 1, 0, true, false);
    if (!bad.empty()) return "32-bit program: " + bad;
    std::vector<int> at;
    plk_v4t_candidates(in, nchar, at);
    const size_t per = plk_v4t_extra_bytes(nchar);
    if (nchar * nchar * nchar > 256) {
        if (!at.empty()) return "a candidate although the combined code is no byte";
        PlkFusedPT out;
        plk_fused_v4t_build(in, pg.slots_needed, nchar, (size_t)1 << 30, true, out);
        if (out.ntriples != 0 || out.units != in.units || out.words != in.words) return "the form applied although the combined code is no byte";
        if (plk_v4t_plan(in, nchar, 4, 10000000, 256, 0, 2, 0).nodes != 0) return "the plan takes the form although the combined code is no byte";
        g_cases++; g_none++;
        return "";
    }
    /* codes and matrices for the value replay */
    Values v;
    v.nchar = nchar; v.E = N - 1;
    std::uniform_real_distribution<double> U(0.01, 1.0);
    v.M.resize((size_t)(N - 1) * 16);
    for (double &x : v.M) x = U(rng);
    v.defs.resize((size_t)nchar * 4);
    for (double &x : v.defs) x = U(rng);
    const size_t S = 24, Spad = 32;
    std::vector<uint8_t> codes((size_t)N * Spad, 0);
    for (uint8_t &c : codes) c = (uint8_t)(rng() % (unsigned)nchar);
    const std::vector<double> tin = build_tables(in, v);

    const size_t bounds[] = {0, per - 1, per, 2 * per, 3 * per + 5, (size_t)1 << 30};
    for (size_t bound : bounds) {
        PlkFusedPT out;
        plk_fused_v4t_build(in, pg.slots_needed, nchar, bound, true, out);
        const size_t want = std::min(at.size(), bound / per);
        if ((size_t)out.ntriples != want) return plk_fmt("%ld three-leaf tables, the bound takes %ld", out.ntriples, (long)want);
        g_cases++;
        if (want == 0) {
            if (out.units != in.units || out.words != in.words || out.mat_edge != in.mat_edge) return "no node taken, but the formats changed";
            g_none++;
            continue;
        }
        g_tables += out.ntriples;
        bad = plk_fused_check_v4t(N, t.ip.data(), t.ix.data(), in, out, nchar);
        if (!bad.empty()) return bad;
        if (out.mat_edge.size() + want != in.mat_edge.size()) return "the matrix stream did not shrink by the absorbed nodes";
        if ((size_t)out.units * nchar * 32 != (size_t)in.units * nchar * 32 + want * per) return "LDS bytes of the rewritten image";
        if (out.row_node.size() + want != in.row_node.size()) return "staged rows of the rewritten program";
        if (scale_positions(out) != scale_positions(in)) return "a SCALE moved";
        for (size_t q = 0; q < out.tab_unit.size(); q++)
            if (out.tab_el[q] >= 0 && (out.tab_edge[q] < 0 || t.ix[out.tab_edge[q]] == t.pre[0])) return "the root was absorbed";
        /* the first `want` candidates, in program order */
        {
            size_t k = 0;
            for (size_t q = 0; q < out.tab_unit.size(); q++) if (out.tab_el[q] >= 0) { if (out.tab_edge[q] != in.vops[at[k] + 2].edge) return "nodes not taken in program order"; k++; }
        }
        for (int C = 1; C <= 4; C++)
            for (int G : {1, 2, C}) {
                if (G > C) continue;
                const int Cg = (C + G - 1) / G;
                const size_t lds = plk_fused_v4s_lds_bytes(out, nchar, Cg);
                if (lds > plk_pt_lds_limit(1024)) continue;
                PlkK4Stream st;
                PlkFusedV4S &vs = st.fv4s, vin;
                plk_fused_v4s_words(out, nchar, C, 0, vs, Cg);
                bad = plk_fused_check_v4s(out, vs, nchar, C, 0, lds);
                if (!bad.empty()) return plk_fmt("C %ld in %ld groups: ", C, G) + bad;
                plk_fused_v4s_words(in, nchar, C, 0, vin);
                if (vs.nobs + (int)want != vin.nobs || vs.chunks > vin.chunks) return "observations of the rewritten stream";
                /* one image too few must be refused */
                if (Cg > 1 && plk_fused_check_v4s(out, vs, nchar, C, 0, lds - 32).empty()) return "a launch with too little LDS was accepted";
                /* what the engine derives from this stream: the fold, and within 3 stack slots the pair products, each replayed */
                st.held = true;
                plk_k4_stream_fold_pair(st, true, pg.slots_needed <= PLK_V4P_STACK_SLOTS);
                if (!st.note.empty()) return st.note;
                if (st.runs == PlkK4Stream::CHECKED) return "the fold of the rewritten stream does not run";
            }
        const std::vector<double> tout = build_tables(out, v);
        if (!same_values(in, out, v, tin, tout, codes, Spad, S)) return "the rewritten program computes other bits than the checked one";

        if (!controls || bound != ((size_t)1 << 30)) continue;
        /* 1: wrong code radix in the table */
        if (nchar > 1) {
            if (same_values(in, out, v, tin, build_tables(out, v, true), codes, Spad, S)) return "control: a table laid out with the wrong radix gives the same bits";
            g_ctl[0]++;
        }
        int tq = -1;
        for (size_t q = 0; q < out.tab_unit.size(); q++) if (out.tab_el[q] >= 0) { tq = (int)q; break; }
        /* 2: the absorbed matrix left in the stream */
        {
            PlkFusedPT m = out;
            m.mat_edge = in.mat_edge;
            if (plk_fused_check_v4t(N, t.ip.data(), t.ix.data(), in, m, nchar).empty()) return "control: an absorbed matrix left in the stream was accepted";
            g_ctl[1]++;
        }
        /* 3: a SCALE dropped */
        for (size_t i = 0; i < out.vops.size(); i++)
            if (out.vops[i].code == OP_SCALE) {
                PlkFusedPT m = out;
                m.vops.erase(m.vops.begin() + (long)i);
                plk_fused_pt_words(pg.slots_needed, true, m);
                if (plk_fused_check_v4t(N, t.ip.data(), t.ix.data(), in, m, nchar).empty()) return "control: a dropped SCALE was accepted";
                g_ctl[2]++;
                break;
            }
        /* 5: the cherry's leaves swapped in the row only */
        for (size_t r = 0; r < out.row_node.size(); r++)
            if (out.row_node3[r] >= 0) {
                PlkFusedPT m = out;
                std::swap(m.row_node[r], m.row_node2[r]);
                if (plk_fused_check_v4t(N, t.ip.data(), t.ix.data(), in, m, nchar).empty()) return "control: a row with the cherry's leaves swapped was accepted";
                if (same_values(in, m, v, tin, tout, codes, Spad, S)) return "control: a row with the cherry's leaves swapped gives the same bits";
                g_ctl[4]++;
                break;
            }
        /* 6: the row built from the next edge's matrix */
        if (!out.mat_edge.empty()) {
            PlkFusedPT m = out;
            size_t nm = 0;
            for (const PlkFusedPT::VOp &o : out.vops) {
                if (o.code == OP_TIP_SET && o.unit == out.tab_unit[tq]) break;
                if (o.code == OP_MATVEC) nm++;
            }
            if (nm < out.mat_edge.size()) {
                m.tab_edge[tq] = out.mat_edge[nm];
                if (plk_fused_check_v4t(N, t.ip.data(), t.ix.data(), in, m, nchar).empty()) return "control: a table of the next edge was accepted";
                if (same_values(in, m, v, tin, build_tables(m, v), codes, Spad, S)) return "control: a table of the next edge gives the same bits";
                g_ctl[5]++;
            }
        }
    }
    /* 4: the root's cherry and leaf absorbed (the last two look-ups of the program with no MATVEC behind them) */
    if (controls && in.vops.size() >= 2) {
        const size_t i = in.vops.size() - 2;
        std::vector<int> table_at(std::max(in.units, 1), -1);
        for (size_t q = 0; q < in.tab_unit.size(); q++) table_at[in.tab_unit[q]] = (int)q;
        if (in.vops[i].code == OP_TIP_SET && in.vops[i + 1].code == OP_TIP_MUL && in.tab_eb[table_at[in.vops[i].unit]] >= 0 &&
            in.tab_eb[table_at[in.vops[i + 1].unit]] < 0 && in.tab_edge[table_at[in.vops[i + 1].unit]] >= 0) {
            /* a builder that takes the node although nothing stands above it: the table gets the cherry's own edge */
            PlkFusedPT m;
            const int tp = table_at[in.vops[i].unit], tl = table_at[in.vops[i + 1].unit];
            m.vops.assign(in.vops.begin(), in.vops.begin() + (long)i);
            m.tab_unit = in.tab_unit; m.tab_edge = in.tab_edge; m.tab_eb = in.tab_eb; m.tab_ec = in.tab_ec;
            m.tab_ea.assign(in.tab_unit.size(), -1); m.tab_el.assign(in.tab_unit.size(), -1);
            m.row_node = in.row_node; m.row_node2 = in.row_node2; m.row_node3.assign(in.row_node.size(), -1);
            m.mat_edge = in.mat_edge; m.units = in.units; m.npairs = in.npairs;
            m.tab_unit.push_back(m.units); m.tab_edge.push_back(in.tab_edge[tp]); m.tab_eb.push_back(in.tab_eb[tp]); m.tab_ec.push_back(in.tab_ec[tp]);
            m.tab_ea.push_back(in.tab_edge[tp]); m.tab_el.push_back(in.tab_edge[tl]);
            m.row_node.push_back(in.row_node[in.vops[i].row]); m.row_node2.push_back(in.row_node2[in.vops[i].row]); m.row_node3.push_back(in.row_node[in.vops[i + 1].row]);
            m.vops.push_back(PlkFusedPT::VOp{OP_TIP_SET, m.units, (int)m.row_node.size() - 1, 0, -1});
            m.units += nchar * nchar; m.ntriples = 1;
            if (m.units < 2048) {
                plk_fused_pt_words(pg.slots_needed, true, m);
                if (plk_fused_check_v4t(N, t.ip.data(), t.ix.data(), in, m, nchar).empty()) return "control: the root as a three-leaf table was accepted";
                g_ctl[3]++;
            }
        }
    }
    return "";
}

int main(int argc, char **argv)
{
    std::mt19937 rng(20240521u);
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        Tree t;
        if (!f || fscanf(f, "%d", &t.N) != 1 || t.N < 2 || t.N > 100000) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
        t.ip.resize(t.N + 1); t.ix.resize(t.N - 1); t.pre.resize(t.N);
        bool ok = true;
        for (int &x : t.ip) ok = ok && fscanf(f, "%d", &x) == 1;
        for (int &x : t.ix) ok = ok && fscanf(f, "%d", &x) == 1;
        for (int &x : t.pre) ok = ok && fscanf(f, "%d", &x) == 1;
        fclose(f);
        if (!ok) { fprintf(stderr, "short tree file\n"); return 1; }
        const std::string bad = check_tree(t, 5, rng, true);
        if (!bad.empty()) { fprintf(stderr, "config 3: %s\n", bad.c_str()); return 1; }
        std::vector<char> has(t.N, 0);
        PlkProgram pg;
        plk_program_build(t.N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
        PlkFusedPT in, out;
        plk_fused_pt_build(t.N, t.ip.data(), t.ix.data(), pg, 5, 1 << 30, in, true);
        std::vector<int> at;
        plk_v4t_candidates(in, 5, at);
        const PlkV4TPlan g1 = plk_v4t_plan(in, 5, 4, 10000000, 256, 0, 2, 1), g2 = plk_v4t_plan(in, 5, 4, 10000000, 256, 0, 2, 2),
                         gc = plk_v4t_plan(in, 5, 4, 10000000, 256, 0, 2, -1), dflt = plk_v4t_plan(in, 5, 4, 10000000, 256, 0, 1, 0),
                         small = plk_v4t_plan(in, 5, 4, 300, 256, 0, 1, 0);
        plk_fused_v4t_build(in, pg.slots_needed, 5, g2.extra_bytes, true, out);
        /* what the engine's plan is handed: plk_k4_choose's, the same function of the shape */
        {
            PlkFused fu; PlkFusedPT fpt; PlkFusedV4 fv4; PlkFusedV4S fv4s;
            auto chosen = [&](long S, long option) {
                PlkK4Shape sh = {5, 4, S, 256, option, 1, 0, {0, 0, 0}};
                return plk_k4_choose(t.N, t.ip.data(), t.ix.data(), pg, sh, true, fu, fpt, fv4, fv4s);
            };
            const PlkK4Choice big = chosen(10000000, 1), little = chosen(300, 1), off = chosen(10000000, 1 + 2048), nopair = chosen(10000000, 1 + 1024 + 512);
            if (!big.bad.empty() || big.variant != PLK_K4_V4S || big.triple.groups != dflt.groups || big.triple.nodes != dflt.nodes || big.triple.Cg != dflt.Cg)
                { fprintf(stderr, "config 3: plk_k4_choose and plk_v4t_plan disagree\n"); return 1; }
            if (little.triple.nodes != 0 || off.triple.nodes != 0) { fprintf(stderr, "config 3: the form at 300 sites or under + 2048\n"); return 1; }
            if (nopair.triple.groups != 1 || nopair.triple.nodes != g1.nodes) { fprintf(stderr, "config 3: groups without the pair-product form\n"); return 1; }
        }
        if (g1.groups != 1 || g2.groups != 2 || gc.groups != 4 || g2.Cg != 2 || gc.Cg != 1) { fprintf(stderr, "config 3: groups of the forced plans\n"); return 1; }
        printf("config3 %d %d %d %d %d %d %d %d %d %d\n", (int)at.size(), in.units, (int)in.mat_edge.size(), g1.nodes, g2.nodes, gc.nodes,
               (int)out.mat_edge.size(), dflt.groups, dflt.nodes, small.nodes);
    }
    const int nchars[] = {4, 5, 6, 7, 16};
    for (int leaves = 3; leaves <= 12; leaves++)
        for (int balanced = 0; balanced < 2; balanced++)
            for (int flip = 0; flip < 2; flip++)
                for (int nchar : nchars) {
                    Tree t;
                    if (!shaped_tree(leaves, balanced != 0, flip != 0, t)) { fprintf(stderr, "tree generator\n"); return 1; }
                    const std::string bad = check_tree(t, nchar, rng, true);
                    if (!bad.empty()) { fprintf(stderr, "%d leaves, balanced %d, flipped %d, nchar %d: %s\n", leaves, balanced, flip, nchar, bad.c_str()); return 1; }
                }
    for (int flip = 0; flip < 2; flip++) {
        Tree t;
        if (!shaped_tree(40, false, flip != 0, t)) { fprintf(stderr, "tree generator\n"); return 1; }
        const std::string bad = check_tree(t, 4, rng, true);
        if (!bad.empty()) { fprintf(stderr, "40-leaf caterpillar, flipped %d: %s\n", flip, bad.c_str()); return 1; }
    }
    printf("ok %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", g_cases, g_tables, g_none, g_ctl[0], g_ctl[1], g_ctl[2], g_ctl[3], g_ctl[4], g_ctl[5]);
    return 0;
}
