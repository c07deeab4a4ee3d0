/*
 * tests/quadcheck_main.cpp -- CPU driver for the FOUR-LEAF TABLES of the streamed k = 4 interpreter (plk_v4q_candidates,
 * plk_fused_v4q_build, plk_fused_check_v4q, plk_v4q_lut / plk_v4q_rank_codes, plk_v4q_plan and the four-node rows of
 * plk_stream_site_dword in phyly_amd/csrc/plk_program.h), built with AddressSanitizer + UBSan by tests/test_k4_quad_host.py.
 *
 * Shapes (nested brackets, 0 = a leaf): the two five-leaf shapes ((((0,0),0),0),0) (shape A) and (((0,0),(0,0)),0) (shape B);
 * the four-leaf trees themselves, where the node is the root (no candidate); what follows the absorbed product (TIP_MUL,
 * MATVEC of a unary node, PUSH, POPMUL); a third child at d; a 40-leaf caterpillar (the SCALE ops stay); data at d; a leaf
 * with five occurring codes (no four-leaf table: the three-leaf table is taken instead); random binary trees.  Occurring
 * codes: nchar 4, 5 and 16, contiguous and not ({1, 5, 9, 15}), another subset at every leaf, a leaf with one code, leaves
 * at which code 0 never occurs (the padded sites must land on rank 0).  For every case:
 *   - the rewritten formats replay (plk_fused_check_v4q, then plk_fused_check_v4s, the fold and the pair-product derivation
 *     on their streamed words, in 1, 2 and C groups);
 *   - no table stands for the root, the SCALE ops sit where they sat, the matrix stream shrinks by two per shape A, one per
 *     shape B and one per three-leaf table, a table is 256 rows in ceil(256 / nchar) units;
 *   - VALUES: with random fp64 matrices, tables of both formats built on the host (a four-leaf row by plk_v4t_row twice /
 *     once, the function the device builder calls, over the codes plk_v4q_rank_codes names) and codes drawn from every
 *     leaf's occurring set, read back through plk_stream_site_dword with the rank tables, a host interpreter of the
 *     handlers' fp64 sequences gives the root vector of the rewritten program bit for bit as the checked program's.
 * Controls that must fail: the replay check refuses a row with two leaves swapped, one wrong rank-table entry, an absorbed
 * matrix left in the stream and a table one unit short; the value replay refuses rows built in double-double and rounded
 * once (required wherever every leaf of the four-leaf rows takes at least two codes, so that the sites read 16 or more
 * distinct rows; with a single-code leaf the sites may read one row, whose four entries can round alike: counted), rows
 * with e_t and e_d swapped, and rows in which the second leaf is multiplied in before the inner product.
 * A SCALE inside the run: plk_program_build never puts one there (a node is rescaled after 16 accumulated factors), so the
 * case is made by hand -- an OP_SCALE inserted into the checked ops before MATVEC(e_t), before MATVEC(e_d) (shape A) and
 * between POPMUL and MATVEC (shape B): no candidate at that index, the builder handed the index leaves the ops as they
 * are, and formats with the four-leaf table forced over such a run are refused by the replay check.
 * With a file name as argument (the tree of BASELINE config 3 as tests/foldcheck_main.cpp reads it; nchar 5, C 4, every
 * leaf taking codes 0 .. 3) it prints "config3 <four-leaf candidates A> <B> <groups> <four-leaf tables> <three-leaf tables>
 * <units> <matrices left> <observations> <four-leaf tables at 300 sites> <under + 1024 alone> <under + 32768>" from the plan at
 * 10M sites, 256 CUs and 4608 B of static LDS.
 * Prints "ok <cases> <shape A tables> <shape B tables> <three-leaf tables beside them> <controls: swap lut matrix short
 * dd edges order scale>" and exits 0, or the first failure and exits 1.
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

/* "((0,0),0)" -> a tree; a node may have any number of children */
static int parse(const char *&s, int &next, std::vector<int> &ea, std::vector<int> &eb)
{
    const int me = next++;
    if (*s == '0') { s++; return me; }
    s++;                                  /* ( */
    while (*s != ')') {
        if (*s == ',') { s++; continue; }
        const int c = parse(s, next, ea, eb);
        ea.push_back(me); eb.push_back(c);
    }
    s++;
    return me;
}
static bool shape_tree(const char *shape, Tree &t)
{
    std::vector<int> ea, eb;
    int next = 0;
    parse(shape, next, ea, eb);
    return make_tree(next, ea, eb, t);
}
/* a random binary tree over `leaves` leaves */
static int grow(int leaves, std::mt19937 &rng, int &next, std::vector<int> &ea, std::vector<int> &eb)
{
    const int me = next++;
    if (leaves == 1) return me;
    const int left = 1 + (int)(rng() % (unsigned)(leaves - 1));
    const int a = grow(left, rng, next, ea, eb), b = grow(leaves - left, rng, next, ea, eb);
    ea.push_back(me); eb.push_back(a); ea.push_back(me); eb.push_back(b);
    return me;
}

static long g_cases = 0, g_A = 0, g_B = 0, g_tri = 0, g_ctl[8] = {0, 0, 0, 0, 0, 0, 0, 0};

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
/* the row in double-double, as the pair and tip tables are built, rounded once at the end: what the four-leaf rows must NOT be */
struct DD { double hi, lo; };
static DD dd_two_sum(double a, double b) { const double s = a + b, bb = s - a; return DD{s, (a - (s - bb)) + (b - bb)}; }
static DD dd_two_prod(double a, double b) { const double p = a * b; return DD{p, fma(a, b, -p)}; }
static DD dd_add(DD a, DD b) { DD s = dd_two_sum(a.hi, b.hi); s.lo += a.lo + b.lo; return dd_two_sum(s.hi, s.lo); }
static DD dd_mul_d(DD a, double b) { DD p = dd_two_prod(a.hi, b); p.lo += a.lo * b; return dd_two_sum(p.hi, p.lo); }
static void row_dd(const double *M, const double *a, const double *b, double *out)
{
    for (int i = 0; i < 4; i++) {
        DD acc{0.0, 0.0};
        for (int j = 0; j < 4; j++) acc = dd_add(acc, dd_mul_d(dd_two_prod(a[j], b[j]), M[4 * j + i]));
        out[i] = acc.hi;
    }
}

enum { BUG_NONE = 0, BUG_DD, BUG_EDGES, BUG_ORDER };

static std::vector<double> build_tables(const PlkFusedPT &f, const Values &v, const std::vector<int> &node_codes, int bug = BUG_NONE)
{
    const int n = v.nchar;
    std::vector<double> tab((size_t)f.units * n * 4, 0.0);
    auto mat = [&](int e) { return &v.M[(size_t)e * 16]; };
    for (size_t t = 0; t < f.tab_unit.size(); t++) {
        double *out = &tab[(size_t)f.tab_unit[t] * n * 4];
        const int shape = t < f.tab_shape.size() ? f.tab_shape[t] : 0;
        const bool tri = !shape && t < f.tab_el.size() && f.tab_el[t] >= 0;
        if (shape) {
            /* the row that reads the table (PlkFusedPT::tab_row, as the engine finds it) names the leaves, and through them the
             * codes behind the ranks */
            const int row = f.tab_row[t];
            const int nd[4] = {f.row_node[row], f.row_node2[row], f.row_node3[row], f.row_node4[row]};
            int code[4][4];
            for (int j = 0; j < 4; j++) plk_v4q_rank_codes(node_codes[nd[j]], code[j]);
            for (int idx = 0; idx < PLK_V4Q_ROWS; idx++) {
                const int r1 = idx >> 6, r2 = (idx >> 4) & 3, r3 = (idx >> 2) & 3, r4 = idx & 3;
                double p[4], q[4], l1[4], l2[4], tt[4];
                pair_row(v, f.tab_ea[t], f.tab_eb[t], f.tab_ec[t], code[0][r1], code[1][r2], p);
                if (shape == PLK_V4Q_A) {
                    single_row(v, f.tab_el[t], code[2][r3], l1); single_row(v, f.tab_ef[t], code[3][r4], l2);
                    const double *Mt = mat(bug == BUG_EDGES ? f.tab_edge[t] : f.tab_et[t]), *Md = mat(bug == BUG_EDGES ? f.tab_et[t] : f.tab_edge[t]);
                    if (bug == BUG_ORDER) {
                        /* (pair o l1 o l2) through both matrices: the second leaf before the inner product */
                        double x[4];
                        for (int j = 0; j < 4; j++) x[j] = p[j] * l2[j];
                        plk_v4t_row(Mt, x, l1, tt);
                        double one[4] = {1.0, 1.0, 1.0, 1.0};
                        plk_v4t_row(Md, tt, one, out + (size_t)idx * 4);
                    } else if (bug == BUG_DD) { row_dd(Mt, p, l1, tt); row_dd(Md, tt, l2, out + (size_t)idx * 4); }
                    else { plk_v4t_row(Mt, p, l1, tt); plk_v4t_row(Md, tt, l2, out + (size_t)idx * 4); }
                } else {
                    pair_row(v, f.tab_et[t], f.tab_ef[t], f.tab_eg[t], code[2][r3], code[3][r4], q);
                    if (bug == BUG_DD) row_dd(mat(f.tab_edge[t]), p, q, out + (size_t)idx * 4);
                    else plk_v4t_row(mat(bug == BUG_EDGES ? f.tab_et[t] : f.tab_edge[t]), p, q, out + (size_t)idx * 4);
                }
            }
        } else if (tri) {
            for (int cb = 0; cb < n; cb++) for (int cc = 0; cc < n; cc++) for (int cl = 0; cl < n; cl++) {
                double p[4], l[4];
                pair_row(v, f.tab_ea[t], f.tab_eb[t], f.tab_ec[t], cb, cc, p);
                single_row(v, f.tab_el[t], cl, l);
                plk_v4t_row(mat(f.tab_edge[t]), p, l, out + (size_t)((cb * n + cc) * n + cl) * 4);
            }
        } else if (f.tab_eb[t] >= 0) {
            for (int cb = 0; cb < n; cb++) for (int cc = 0; cc < n; cc++) pair_row(v, f.tab_edge[t], f.tab_eb[t], f.tab_ec[t], cb, cc, out + (size_t)(cb * n + cc) * 4);
        } else for (int code = 0; code < n; code++) single_row(v, f.tab_edge[t], code, out + (size_t)code * 4);
    }
    return tab;
}

/* [5][nrows] as the engine uploads them */
static std::vector<int> row_lists(const PlkFusedPT &f)
{
    const size_t nrows = f.row_node.size();
    std::vector<int> rn(5 * nrows, -1);
    for (size_t r = 0; r < nrows; r++) {
        rn[r] = f.row_node[r]; rn[nrows + r] = f.row_node2[r];
        if (r < f.row_node3.size()) rn[2 * nrows + r] = f.row_node3[r];
        if (r < f.row_node4.size()) { rn[3 * nrows + r] = f.row_node4[r]; rn[4 * nrows + r] = f.row_lut[r]; }
    }
    return rn;
}

/* the root vector of one site: look-ups through the code stream's bytes, MATVEC as tools/gen_fused4_v4.py emits it */
static bool run_site(const PlkFusedPT &f, const Values &v, const std::vector<double> &tab, const std::vector<uint8_t> &codes, size_t Spad, size_t site, double *root)
{
    const int n = v.nchar, nrows = (int)f.row_node.size();
    std::vector<int> obs_row;
    const std::vector<int> rn = row_lists(f);
    for (const PlkFusedPT::VOp &o : f.vops) if (o.code == OP_TIP_SET || o.code == OP_TIP_MUL) obs_row.push_back(o.row);
    double cur[4] = {0, 0, 0, 0}, slot[4][4];
    int oi = 0;
    size_t mi = 0;
    for (const PlkFusedPT::VOp &o : f.vops) {
        if (o.code == OP_TIP_SET || o.code == OP_TIP_MUL) {
            const unsigned d = plk_stream_site_dword(codes.data(), Spad, site, obs_row.data(), (int)obs_row.size(), rn.data(), nrows, n, oi / 4, 5,
                                                     f.lut.empty() ? nullptr : f.lut.data());
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
    std::vector<int> len(std::max(f.units, 1), 1);
    for (size_t t = 0; t < f.tab_unit.size(); t++) {
        if (t < f.tab_shape.size() && f.tab_shape[t]) len[f.tab_unit[t]] = 5;
        else if (t < f.tab_el.size() && f.tab_el[t] >= 0) len[f.tab_unit[t]] = 3;
    }
    for (const PlkFusedPT::VOp &o : f.vops) {
        if (o.code == OP_SCALE) at.push_back(n);
        n += (o.code == OP_TIP_SET || o.code == OP_TIP_MUL) ? len[o.unit] : 1;
    }
    return at;
}

/* occurring codes per node: kind 0 codes 0 .. 3, 1 {1, 5, 9, 15} & nchar, 2 a subset that differs from leaf to leaf, without
 * code 0 at every other leaf, 3 a single code at the first leaf; internal nodes carry the last code ("missing") */
static std::vector<int> make_masks(const Tree &t, int nchar, int kind, std::mt19937 &rng)
{
    std::vector<int> m(t.N, 1 << (nchar - 1));
    int leafno = 0;
    for (int a = 0; a < t.N; a++) {
        if (t.ip[a + 1] != t.ip[a]) continue;
        int mask = 0;
        if (kind == 0) mask = 0xf;
        else if (kind == 1) { const int c[4] = {1, 5, 9, 15}; for (int x : c) if (x < nchar) mask |= 1 << x; if (!mask) mask = 2; if (nchar < 16) mask |= 1 << (nchar - 1); }
        else {
            const int want = kind == 3 && leafno == 0 ? 1 : 1 + (int)(rng() % 4u);
            while (plk_popcount16(mask) < std::min(want, nchar - (leafno & 1))) { const int c = (int)(rng() % (unsigned)nchar); if (c == 0 && (leafno & 1)) continue; mask |= 1 << c; }
        }
        m[a] = mask & ((1 << nchar) - 1);
        leafno++;
    }
    return m;
}

/* expect_A / expect_B: -1 = whatever */
static std::string check_tree(const Tree &t, int nchar, const std::vector<int> &masks, const std::vector<char> &has, std::mt19937 &rng, bool controls,
                              int expect_A, int expect_B, int expect_tri)
{
    const int N = t.N;
    PlkProgram pg;
    plk_program_build(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
    std::string bad = plk_program_check(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
    if (!bad.empty()) return bad;
    if (pg.slots_needed > 4) return "";
    PlkFusedPT in;
    plk_fused_pt_build(N, t.ip.data(), t.ix.data(), pg, nchar, 1 << 30, in, true);
    bad = plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, in, nchar, 1, 0, true, false);
    if (!bad.empty()) return "32-bit program: " + bad;
    std::vector<PlkV4QCand> qc;
    std::vector<int> tc;
    plk_v4q_candidates(in, nchar, masks.data(), qc);
    plk_v4t_candidates(in, nchar, tc);
    int nA = 0, nB = 0;
    std::vector<int> qat, qsh, tri;
    for (const PlkV4QCand &c : qc) { (c.shape == PLK_V4Q_A ? nA : nB)++; qat.push_back(c.at); qsh.push_back(c.shape); }
    for (int a : tc) if (std::find(qat.begin(), qat.end(), a) == qat.end()) tri.push_back(a);
    if ((expect_A >= 0 && nA != expect_A) || (expect_B >= 0 && nB != expect_B)) return plk_fmt("%ld shape-A and %ld shape-B candidates", nA, nB);
    if (expect_tri >= 0 && (int)tri.size() != expect_tri) return plk_fmt("%ld three-leaf candidates beside the four-leaf ones", (long)tri.size());
    g_cases++;
    PlkFusedPT out;
    plk_fused_v4q_build(in, pg.slots_needed, nchar, masks.data(), tri, qat, qsh, true, out);
    if (out.nquads != nA + nB || out.ntriples != (int)tri.size()) return "the builder took other nodes than it was handed";
    if (out.units >= 2048) return "";
    if (qc.empty()) {
        if (tri.empty() && (out.units != in.units || out.words != in.words || out.mat_edge != in.mat_edge)) return "no node taken, but the formats changed";
        if (tri.empty()) return "";
    }
    g_A += nA; g_B += nB; g_tri += (long)tri.size();
    bad = plk_fused_check_v4q(N, t.ip.data(), t.ix.data(), in, out, nchar, masks.data());
    if (!bad.empty()) return bad;
    if (out.mat_edge.size() + 2 * (size_t)nA + (size_t)nB + tri.size() != in.mat_edge.size()) return "the matrix stream did not shrink by the absorbed products";
    const long U4 = plk_v4q_units(nchar);
    if (U4 * nchar < 256 || (U4 - 1) * nchar >= 256) return "units of a four-leaf table";
    if ((long)out.units != (long)in.units + nA * (U4 - nchar - 2) + nB * (U4 - 2 * nchar) + (long)tri.size() * (nchar * nchar - nchar - 1)) return "units of the rewritten image";
    if (scale_positions(out) != scale_positions(in)) return "a SCALE moved";
    for (size_t q = 0; q < out.tab_unit.size(); q++)
        if (out.tab_shape[q] && (out.tab_edge[q] < 0 || t.ix[out.tab_edge[q]] == t.pre[0])) return "the root was absorbed";
    for (int C = 1; C <= 4; C++)
        for (int G : {1, 2, C}) {
            if (G > C) continue;
            const int Cg = (C + G - 1) / G;
            const size_t lds = plk_fused_v4s_lds_bytes(out, nchar, Cg);
            if (lds > plk_pt_lds_limit(1024)) continue;
            PlkK4Stream st;
            PlkFusedV4S &vs = st.fv4s;
            plk_fused_v4s_words(out, nchar, C, 0, vs, Cg);
            bad = plk_fused_check_v4s(out, vs, nchar, C, 0, lds);
            if (!bad.empty()) return plk_fmt("C %ld in %ld groups: ", C, G) + bad;
            if (Cg > 1 && plk_fused_check_v4s(out, vs, nchar, C, 0, lds - 32).empty()) return "a launch with too little LDS was accepted";
            /* what the engine derives from this stream: the fold, and within 3 stack slots the pair products, each replayed */
            st.held = true;
            plk_k4_stream_fold_pair(st, true, pg.slots_needed <= PLK_V4P_STACK_SLOTS);
            if (!st.note.empty()) return st.note;
            if (st.runs == PlkK4Stream::CHECKED) return "the fold of the rewritten stream does not run";
        }
    /* values */
    Values v;
    v.nchar = nchar; v.E = N - 1;
    std::uniform_real_distribution<double> U(0.01, 1.0);
    v.M.resize((size_t)(N - 1) * 16);
    for (double &x : v.M) x = U(rng);
    v.defs.resize((size_t)nchar * 4);
    for (double &x : v.defs) x = U(rng);
    const size_t S = 40, Spad = 48;
    std::vector<uint8_t> codes((size_t)N * Spad, 0);
    for (int a = 0; a < N; a++) {
        int list[16], n = 0;
        for (int c = 0; c < 16; c++) if ((masks[a] >> c) & 1) list[n++] = c;
        for (size_t s = 0; s < S; s++) codes[(size_t)a * Spad + s] = (uint8_t)list[s < (size_t)n ? s : rng() % (unsigned)n];     /* every occurring code occurs */
    }
    const std::vector<double> tin = build_tables(in, v, masks), tout = build_tables(out, v, masks);
    if (!same_values(in, out, v, tin, tout, codes, Spad, S)) return "the rewritten program computes other bits than the checked one";
    /* padded sites carry code 0 at every node: every digit of a four-leaf byte is then the rank of code 0, or 0 where it does not occur */
    {
        std::vector<int> obs_row;
        const std::vector<int> rn = row_lists(out);
        for (const PlkFusedPT::VOp &o : out.vops) if (o.code == OP_TIP_SET || o.code == OP_TIP_MUL) obs_row.push_back(o.row);
        for (size_t n = 0; n < obs_row.size(); n++) {
            const int r = obs_row[n];
            if (out.row_lut[r] < 0) continue;
            const unsigned d = plk_stream_site_dword(codes.data(), Spad, S + 3, obs_row.data(), (int)obs_row.size(), rn.data(), (int)out.row_node.size(), nchar, (int)n / 4, 5, out.lut.data());
            const unsigned byte = (d >> (8 * (n % 4))) & 0xffu;
            const int nd[4] = {out.row_node[r], out.row_node2[r], out.row_node3[r], out.row_node4[r]};
            for (int j = 0; j < 4; j++) if (((byte >> (2 * (3 - j))) & 3u) != 0u) return "a padded site does not land on rank 0";
            (void)nd;
        }
    }
    if (!controls || qc.empty()) return "";
    int rq = -1, tq = -1;
    for (size_t r = 0; r < out.row_node.size(); r++) if (out.row_lut[r] >= 0) { rq = (int)r; break; }
    for (size_t q = 0; q < out.tab_unit.size(); q++) if (out.tab_shape[q]) { tq = (int)q; break; }
    /* 0: two leaves swapped in the row only (the second and the third: across the cherry's border) */
    {
        PlkFusedPT m = out;
        std::swap(m.row_node2[rq], m.row_node3[rq]);
        if (plk_fused_check_v4q(N, t.ip.data(), t.ix.data(), in, m, nchar, masks.data()).empty()) return "control: a row with two leaves swapped was accepted";
        g_ctl[0]++;
    }
    /* 1: one wrong rank-table entry (an occurring code of the first leaf sent to another rank) */
    {
        PlkFusedPT m = out;
        int code = 0;
        while (!((masks[out.row_node[rq]] >> code) & 1)) code++;
        m.lut[(size_t)64 * out.row_lut[rq] + code] ^= 1;
        if (plk_fused_check_v4q(N, t.ip.data(), t.ix.data(), in, m, nchar, masks.data()).empty()) return "control: a wrong rank-table entry was accepted";
        /* ... and an entry of a code that does not occur, which must stay 0 */
        m = out;
        for (code = 0; code < 16 && ((masks[out.row_node[rq]] >> code) & 1); code++) {}
        if (code < 16) {
            m.lut[(size_t)64 * out.row_lut[rq] + code] = 1;
            if (plk_fused_check_v4q(N, t.ip.data(), t.ix.data(), in, m, nchar, masks.data()).empty()) return "control: a rank for a code that does not occur was accepted";
        }
        g_ctl[1]++;
    }
    /* 2: the absorbed matrices left in the stream */
    {
        PlkFusedPT m = out;
        m.mat_edge = in.mat_edge;
        if (plk_fused_check_v4q(N, t.ip.data(), t.ix.data(), in, m, nchar, masks.data()).empty()) return "control: absorbed matrices left in the stream were accepted";
        g_ctl[2]++;
    }
    /* 3: the table one unit short: everything behind it moves up one unit */
    {
        PlkFusedPT m = out;
        for (size_t q = 0; q < m.tab_unit.size(); q++) if (m.tab_unit[q] > out.tab_unit[tq]) m.tab_unit[q]--;
        for (PlkFusedPT::VOp &o : m.vops) if ((o.code == OP_TIP_SET || o.code == OP_TIP_MUL) && o.unit > out.tab_unit[tq]) o.unit--;
        m.units--;
        plk_fused_pt_words(pg.slots_needed, true, m);
        if (plk_fused_check_v4q(N, t.ip.data(), t.ix.data(), in, m, nchar, masks.data()).empty()) return "control: a four-leaf table one unit short was accepted";
        g_ctl[3]++;
    }
    /* 4 - 6: wrong rows */
    /* double-double rows differ from the handlers' sequence by roundings only: an entry agrees about every other time.  Where
     * every leaf of every four-leaf row takes at least two codes the 40 sites read 16 or more distinct rows (64 entries and
     * more) and a difference is required; where a leaf takes a single code the sites may read one row, four entries, which
     * can agree by chance: counted where it shows */
    {
        int fewest = 4;
        for (size_t r = 0; r < out.row_node.size(); r++) {
            if (out.row_lut[r] < 0) continue;
            const int nd[4] = {out.row_node[r], out.row_node2[r], out.row_node3[r], out.row_node4[r]};
            for (int j = 0; j < 4; j++) fewest = std::min(fewest, plk_popcount16(masks[nd[j]]));
        }
        const bool same = same_values(in, out, v, tin, build_tables(out, v, masks, BUG_DD), codes, Spad, S);
        if (same && fewest >= 2) return "control: rows built in double-double give the same bits";
        if (!same) g_ctl[4]++;
    }
    if (same_values(in, out, v, tin, build_tables(out, v, masks, BUG_EDGES), codes, Spad, S)) return "control: rows with the edges swapped give the same bits";
    g_ctl[5]++;
    if (nA > 0) {
        if (same_values(in, out, v, tin, build_tables(out, v, masks, BUG_ORDER), codes, Spad, S)) return "control: rows with the leaf multiplied before the inner product give the same bits";
        g_ctl[6]++;
    }
    return "";
}

/* A SCALE inside the run, made by hand (the program builder never emits one there): OP_SCALE inserted `off` ops behind the
 * first op of the one candidate of `shape` */
static std::string scale_inside_run(const char *shape, int want_shape, int nchar, std::mt19937 &rng)
{
    typedef PlkFusedPT::VOp VOp;
    Tree t;
    if (!shape_tree(shape, t)) return "tree generator";
    const int N = t.N;
    std::vector<char> has(N, 0);
    const std::vector<int> masks = make_masks(t, nchar, 0, rng);
    PlkProgram pg;
    plk_program_build(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
    PlkFusedPT in, good;
    plk_fused_pt_build(N, t.ip.data(), t.ix.data(), pg, nchar, 1 << 30, in, true);
    std::string bad = plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, in, nchar, 1, 0, true, false);
    if (!bad.empty()) return "32-bit program: " + bad;
    std::vector<PlkV4QCand> qc;
    plk_v4q_candidates(in, nchar, masks.data(), qc);
    if (qc.size() != 1 || qc[0].shape != want_shape) return "the shape has not its one candidate";
    const int at = qc[0].at;
    const std::vector<int> none, qat(1, at), qsh(1, want_shape);
    plk_fused_v4q_build(in, pg.slots_needed, nchar, masks.data(), none, qat, qsh, true, good);
    if (good.nquads != 1 || !(bad = plk_fused_check_v4q(N, t.ip.data(), t.ix.data(), in, good, nchar, masks.data())).empty()) return "without the SCALE: " + bad;
    /* A: before MATVEC(e_t) and before MATVEC(e_d); B: between POPMUL and MATVEC(e_d) */
    const std::vector<int> offs = want_shape == PLK_V4Q_A ? std::vector<int>{2, 4} : std::vector<int>{4};
    for (int off : offs) {
        PlkFusedPT sc = in, out;
        if (sc.vops[at + off].code != OP_MATVEC) return "the run is not where it was expected";
        sc.vops.insert(sc.vops.begin() + at + off, VOp{OP_SCALE, 0, 0, 0, -1});
        plk_fused_pt_words(pg.slots_needed, true, sc);
        plk_v4q_candidates(sc, nchar, masks.data(), qc);
        for (const PlkV4QCand &c : qc) if (c.at >= at - 4 && c.at <= at + 5) return plk_fmt("a candidate although a SCALE stands %ld ops into the run", off);
        plk_fused_v4q_build(sc, pg.slots_needed, nchar, masks.data(), none, qat, qsh, true, out);
        if (out.nquads != 0 || out.ntriples != 0 || out.units != sc.units || out.words != sc.words || out.mat_edge != sc.mat_edge || out.vops.size() != sc.vops.size())
            return plk_fmt("the builder changed the ops although a SCALE stands %ld ops into the run", off);
        for (size_t i = 0; i < sc.vops.size(); i++) {
            const VOp &a = out.vops[i], &b = sc.vops[i];
            if (a.code != b.code || a.unit != b.unit || a.row != b.row || a.d != b.d || a.edge != b.edge) return "the builder changed an op";
        }
        /* the four-leaf table forced over the run: the formats built without the SCALE, set against the program that has it */
        if (plk_fused_check_v4q(N, t.ip.data(), t.ix.data(), sc, good, nchar, masks.data()).empty()) return plk_fmt("control: a four-leaf table over a run with a SCALE %ld ops in was accepted", off);
        /* ... and the same formats with the SCALE kept behind the look-up, where the run's SCALE cannot go */
        PlkFusedPT moved = good;
        for (size_t i = 0; i < moved.vops.size(); i++)
            if (moved.vops[i].code == OP_TIP_SET && moved.row_lut[moved.vops[i].row] >= 0) {
                moved.vops.insert(moved.vops.begin() + (long)i + 1, VOp{OP_SCALE, 0, 0, 0, -1});
                break;
            }
        plk_fused_pt_words(pg.slots_needed, true, moved);
        if (plk_fused_check_v4q(N, t.ip.data(), t.ix.data(), sc, moved, nchar, masks.data()).empty()) return plk_fmt("control: a SCALE moved out of the run (%ld ops in) was accepted", off);
        g_ctl[7]++;
    }
    return "";
}

static int fail(const char *what, const std::string &bad) { fprintf(stderr, "%s: %s\n", what, bad.c_str()); return 1; }

int main(int argc, char **argv)
{
    std::mt19937 rng(20240917u);
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
        std::vector<char> has(t.N, 0);
        std::vector<int> masks(t.N, 1 << 4);
        for (int a = 0; a < t.N; a++) if (t.ip[a + 1] == t.ip[a]) masks[a] = 0xf;
        const std::string bad = check_tree(t, 5, masks, has, rng, true, -1, -1, -1);
        if (!bad.empty()) return fail("config 3", bad);
        PlkProgram pg;
        plk_program_build(t.N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
        PlkFused fu; PlkFusedPT fpt, out; PlkFusedV4 fv4; PlkFusedV4S fv4s;
        auto chosen = [&](long S, long option) {
            PlkK4Shape sh = {5, 4, S, 256, option, 1, 0, {4608, 4608, 4608}};
            sh.node_codes = masks.data();
            return plk_k4_choose(t.N, t.ip.data(), t.ix.data(), pg, sh, true, fu, fpt, fv4, fv4s);
        };
        const PlkK4Choice forced = chosen(10000000, 1 + 16384), little = chosen(300, 1), only3 = chosen(10000000, 1 + 1024), never = chosen(10000000, 1 + 32768);
        if (!forced.bad.empty() || forced.variant != PLK_K4_V4S) return fail("config 3", "the streamed form was not chosen");
        std::vector<PlkV4QCand> qc;
        plk_v4q_candidates(fpt, 5, masks.data(), qc);
        int nA = 0, nB = 0;
        for (const PlkV4QCand &c : qc) (c.shape == PLK_V4Q_A ? nA : nB)++;
        const PlkV4TPlan &tp = forced.triple;
        /* the formats the engine runs under that plan, every capability given (plk_k4_stream builds and replays them) */
        PlkK4Shape shf = {5, 4, 10000000, 256, 1 + 16384, 1, 0, {4608, 4608, 4608}};
        shf.node_codes = masks.data();
        out = fpt;
        const PlkK4Stream run = plk_k4_stream(t.N, t.ip.data(), t.ix.data(), pg, shf, forced, PlkK4StreamCaps(), out, fv4s);
        if (!run.note.empty()) return fail("config 3 plan", run.note);
        if (run.triple.quads != tp.quads || run.triple.nodes != tp.nodes || run.triple.groups != tp.groups) return fail("config 3 plan", "the plan was not taken as chosen");
        const std::string b2 = plk_fused_check_v4q(t.N, t.ip.data(), t.ix.data(), fpt, out, 5, masks.data());
        if (!b2.empty()) return fail("config 3 plan", b2);
        const PlkFusedV4S &vs = run.fv4s;
        const std::string b3 = plk_fused_check_v4s(out, vs, 5, 4, 4608, run.lds);
        if (!b3.empty()) return fail("config 3 stream", b3);
        printf("config3 %d %d %d %d %d %d %d %d %d %d %d\n", nA, nB, tp.groups, out.nquads, out.ntriples, out.units, (int)out.mat_edge.size(), vs.nobs,
               little.triple.quads, only3.triple.quads, never.triple.quads);
    }
    struct Shape { const char *s; int A, B, tri; };
    const Shape shapes[] = {
        {"((((0,0),0),0),0)", 1, 0, 0},            /* shape A, then TIP_MUL */
        {"(((0,0),(0,0)),0)", 0, 1, 0},            /* shape B, then TIP_MUL */
        {"(((0,0),0),0)", 0, 0, 1},                /* the four-leaf node is the root: its three-leaf node stays a candidate */
        {"((0,0),(0,0))", 0, 0, 0},                /* the root again */
        {"(((((0,0),0),0)),0)", 1, 0, 0},          /* then the MATVEC of a unary node */
        {"((((0,0),0),0),(0,0))", 1, 0, 0},        /* then PUSH */
        {"((0,0),(((0,0),0),0))", -1, -1, -1},     /* then POPMUL (whichever child the program visits first) */
        {"((((0,0),(0,0))),0)", 0, 1, 0},          /* shape B, then a unary node's MATVEC */
        {"(((0,0),(0,0)),((0,0),0))", -1, -1, -1}, /* shape B beside a three-leaf node */
        {"((((0,0),0),0,0),0)", 0, 0, 1},          /* a third child at d: the three-leaf node below it only */
        {"(((0,0),(0,0),0),0)", 0, 0, 0},          /* a third child beside two cherries */
        {"(((((0,0),0),0),0),0)", 1, 0, 0},        /* six-leaf caterpillar: the lowest four leaves */
    };
    for (const Shape &sh : shapes)
        for (int nchar : {4, 5, 16})
            for (int kind = 0; kind < 4; kind++) {
                Tree t;
                if (!shape_tree(sh.s, t)) return fail(sh.s, "tree generator");
                std::vector<char> has(t.N, 0);
                const std::vector<int> masks = make_masks(t, nchar, kind, rng);
                /* nchar^3 > 256: no three-leaf candidates at all */
                const std::string bad = check_tree(t, nchar, masks, has, rng, true, sh.A, sh.B, nchar == 16 && sh.tri > 0 ? 0 : sh.tri);
                if (!bad.empty()) { fprintf(stderr, "%s nchar %d codes %d: %s\n", sh.s, nchar, kind, bad.c_str()); return 1; }
            }
    /* a SCALE inside the run */
    for (int nchar : {4, 5, 16}) {
        std::string bad = scale_inside_run("((((0,0),0),0),0)", PLK_V4Q_A, nchar, rng);
        if (bad.empty()) bad = scale_inside_run("(((0,0),(0,0)),0)", PLK_V4Q_B, nchar, rng);
        if (!bad.empty()) return fail("a SCALE inside the run", bad);
    }
    /* a leaf with five occurring codes: no four-leaf table, the three-leaf table instead (nchar 5) */
    for (int which = 0; which < 4; which++) {
        Tree t;
        shape_tree("((((0,0),0),0),0)", t);
        std::vector<char> has(t.N, 0);
        std::vector<int> masks = make_masks(t, 5, 0, rng);
        int leafno = 0;
        for (int a = 0; a < t.N; a++) if (t.ip[a + 1] == t.ip[a] && leafno++ == which) masks[a] = 0x1f;
        const std::string bad = check_tree(t, 5, masks, has, rng, true, 0, 0, 1);
        if (!bad.empty()) return fail("five codes at a leaf", bad);
    }
    /* data at d and at t: another op stands in the run */
    for (int where = 0; where < 2; where++) {
        Tree t;
        shape_tree("((((0,0),0),0),0)", t);
        std::vector<char> has(t.N, 0);
        /* nodes in order of the brackets: 0 root, 1 d, 2 t, 3 the cherry */
        has[where ? 2 : 1] = 1;
        std::vector<int> masks = make_masks(t, 5, 0, rng);
        masks[where ? 2 : 1] = 0xf;
        const std::string bad = check_tree(t, 5, masks, has, rng, true, 0, 0, where ? 0 : 1);
        if (!bad.empty()) return fail("data inside the run", bad);
    }
    /* the 40-leaf caterpillar the program rescales */
    {
        Tree t;
        std::string s = "(0,0)";
        for (int i = 2; i < 40; i++) s = "(" + s + ",0)";
        if (!shape_tree(s.c_str(), t)) return fail("caterpillar", "tree generator");
        std::vector<char> has(t.N, 0);
        const std::string bad = check_tree(t, 4, make_masks(t, 4, 2, rng), has, rng, true, 1, 0, 0);
        if (!bad.empty()) return fail("40-leaf caterpillar", bad);
    }
    /* random trees */
    for (int rep = 0; rep < 120; rep++) {
        std::vector<int> ea, eb;
        int next = 0;
        grow(5 + (int)(rng() % 26u), rng, next, ea, eb);
        Tree t;
        if (!make_tree(next, ea, eb, t)) return fail("random tree", "tree generator");
        std::vector<char> has(t.N, 0);
        const int nchar = rep % 3 == 0 ? 4 : rep % 3 == 1 ? 5 : 16;
        const std::string bad = check_tree(t, nchar, make_masks(t, nchar, rep % 4, rng), has, rng, true, -1, -1, -1);
        if (!bad.empty()) { fprintf(stderr, "random tree %d: %s\n", rep, bad.c_str()); return 1; }
    }
    printf("ok %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", g_cases, g_A, g_B, g_tri, g_ctl[0], g_ctl[1], g_ctl[2], g_ctl[3], g_ctl[4], g_ctl[5], g_ctl[6], g_ctl[7]);
    return 0;
}
