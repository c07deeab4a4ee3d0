/*
 * tests/progcheck_main.cpp -- CPU driver for the traversal-program builder and the host replays of the device
 * interpreters (phyly_amd/csrc/plk_program.h), built with AddressSanitizer + UBSan by tests/test_program_check.py.
 *
 * usage: progcheck                      seeded random trees of every shape the engine accepts
 *        progcheck <file>               trees from a file, one per line: "N nchar  a0 b0 a1 b1 ... | h0 h1 ... hN-1"
 *                                       (edges parent child in user order; h = 1 for nodes that carry data)
 * For every tree: program build + invariants, the rescaling bound (at most PLK_SCALE_RUN edge factors between two OP_SCALE,
 * and the end-of-node rule's program wherever that rule keeps the bound by itself), fused formats for every kernel variant the engine could launch
 * (assembly interpreter with 4-bit and 8-bit codes, C++ interpreter with one and two sites per lane), the chained
 * programs of the three down passes; and negative controls (corrupted words must be refused).
 * Before the trees: a table of site-chunk plans (plk_site_chunk) against the rules the drivers used to spell out inline.
 * Prints "ok <trees> <ops>" and exits 0, or the first failure and exits 1.
 */
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "plk_program.h"

struct Tree { int N; std::vector<int> ip, ix, pre; };

/* CSR + BFS order as host_model.c builds them (src/csr_graph.c:218-229 of the reference: children in user order) */
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

static long g_ops = 0;

/* ------------------------------------------------------------------------------------------------------------ */
/* dynamic range: how many edge factors a vector takes between two rescalings                                     */
/* ------------------------------------------------------------------------------------------------------------ */

/* Replays the program and counts, for cur and for every stack slot, the edge factors multiplied in since the vector's last
 * OP_SCALE: MATVEC, TIP_SET and TIP_MUL add one, POPMUL adds the popped count, SCALE resets.  Returns the largest count any
 * vector reaches.  (The interpreters look at a vector's magnitude at OP_SCALE only, so this is what bounds its range.) */
static int max_unscaled_run(const PlkProgram &pg)
{
    std::vector<int> slot(std::max(pg.slots_needed, 1), 0);
    int cur = 0, worst = 0;
    for (size_t pc = 0; pc < pg.ops.size(); pc++) {
        const int code = pg.ops[pc].x & 0xff, y = pg.ops[pc].y;
        if (code == OP_TIP_SET) cur = 1;
        else if (code == OP_TIP_MUL || code == OP_MATVEC) cur += 1;
        else if (code == OP_PUSH) { slot[y] = cur; cur = 0; }
        else if (code == OP_POPMUL) cur += slot[y];
        else if (code == OP_SCALE) cur = 0;
        worst = std::max(worst, cur);
    }
    return worst;
}

/* The rescaling rule before OP_SCALE could stand inside a node, restated: a node is marked once 16 or more edges have
 * accumulated over ALL its children, and its one OP_SCALE follows its last op.  Same traversal, same op order. */
static void program_build_end_of_node_rule(const Tree &t, const std::vector<char> &has, PlkProgram &pg)
{
    const int N = t.N;
    const int *ip = t.ip.data(), *ix = t.ix.data();
    std::vector<int> need(N, 0), since(N, 0);
    pg.scale_node.assign(N, 0); pg.mid_scale_node.assign(N, 0); pg.mid_scales = 0; pg.wide_node = -1; pg.op_mid.clear();
    std::vector<std::vector<int>> ichild(N);
    for (int u = N - 1; u >= 0; u--) {
        const int a = t.pre[u];
        if (ip[a + 1] == ip[a]) continue;
        std::vector<int> &ic = ichild[a];
        int acc = 0;
        for (int idx = ip[a]; idx < ip[a + 1]; idx++) { acc += since[ix[idx]] + 1; if (ip[ix[idx] + 1] > ip[ix[idx]]) ic.push_back(idx); }
        std::stable_sort(ic.begin(), ic.end(), [&](int x, int y) { return need[ix[x]] > need[ix[y]]; });
        for (size_t i = 0; i < ic.size(); i++) need[a] = std::max(need[a], need[ix[ic[i]]] + (i > 0 ? 1 : 0));
        if (acc >= 16) { pg.scale_node[a] = 1; acc = 0; }
        since[a] = acc;
    }
    pg.slots_needed = need[t.pre[0]];
    pg.ops.clear(); pg.op_edge.clear(); pg.tip_edge.clear(); pg.obs_nodes.clear();
    std::vector<char> staged(N, 0);
    auto obs = [&](int node) { if (!staged[node]) { staged[node] = 1; pg.obs_nodes.push_back(node); } };
    auto emit = [&](int code, int tslot, int arg, int edge) { pg.ops.push_back(plk_op2{code | (tslot << 8), arg}); pg.op_edge.push_back(edge); pg.op_mid.push_back(0); };
    std::function<void(int, int)> go = [&](int a, int depth) {
        const std::vector<int> &ic = ichild[a];
        bool started = false;
        if (!ic.empty()) { go(ix[ic[0]], depth); emit(OP_MATVEC, 0, 0, ic[0]); started = true; }
        for (int idx = ip[a]; idx < ip[a + 1]; idx++) {
            const int b = ix[idx];
            if (ip[b + 1] > ip[b]) continue;
            const int ts = (int)pg.tip_edge.size();
            pg.tip_edge.push_back(idx);
            emit(started ? OP_TIP_MUL : OP_TIP_SET, ts, b, idx);
            obs(b);
            started = true;
        }
        for (size_t i = 1; i < ic.size(); i++) {
            emit(OP_PUSH, 0, depth, -1);
            go(ix[ic[i]], depth + 1);
            emit(OP_MATVEC, 0, 0, ic[i]);
            emit(OP_POPMUL, 0, depth, -1);
        }
        if (has[a]) { emit(OP_NODE_MUL, 0, a, -1); obs(a); }
        if (pg.scale_node[a]) emit(OP_SCALE, 0, a, -1);
    };
    go(t.pre[0], 0);
}

static bool same_program(const PlkProgram &p, const PlkProgram &q)
{
    if (p.ops.size() != q.ops.size() || p.op_edge != q.op_edge || p.tip_edge != q.tip_edge || p.scale_node != q.scale_node ||
        p.obs_nodes != q.obs_nodes || p.slots_needed != q.slots_needed) return false;
    for (size_t i = 0; i < p.ops.size(); i++) if (p.ops[i].x != q.ops[i].x || p.ops[i].y != q.ops[i].y) return false;
    return true;
}

static long g_mid_scaled = 0, g_same_as_before = 0;

/* The bound of the rescaling rule on one tree: no vector takes more than PLK_SCALE_RUN factors between two rescalings; and
 * wherever the end-of-node rule alone keeps that bound -- every tree whose nodes have at most two children among them -- the
 * program is that rule's program op for op, with no OP_SCALE inside a node. */
static std::string check_scale_runs(const Tree &t, const std::vector<char> &has, const PlkProgram &pg)
{
    const int run = max_unscaled_run(pg);
    if (run > PLK_SCALE_RUN) return plk_fmt("rescaling: a vector takes %ld factors between two rescalings (bound %ld)", run, PLK_SCALE_RUN);
    int max_deg = 0;
    for (int a = 0; a < t.N; a++) max_deg = std::max(max_deg, t.ip[a + 1] - t.ip[a]);
    PlkProgram old;
    program_build_end_of_node_rule(t, has, old);
    const int old_run = max_unscaled_run(old);
    if (max_deg <= 2 && old_run > PLK_SCALE_RUN) return "rescaling: the end-of-node rule exceeds its own bound on a tree of degree two";
    if (old_run <= PLK_SCALE_RUN) {
        if (pg.mid_scales != 0 || pg.wide_node >= 0 || !same_program(pg, old)) return "rescaling: the program differs from the end-of-node rule's although that rule keeps the bound";
        g_same_as_before++;
    } else {
        if (pg.mid_scales < 1 || pg.wide_node < 0 || !pg.mid_scale_node[pg.wide_node]) return "rescaling: the end-of-node rule exceeds the bound but no node is rescaled inside";
        g_mid_scaled++;
    }
    return "";
}

/* Invariants of PlkStorageMaps: edge_tip / edge_int partition the edges; node_int >= 0 exactly for the nodes with children;
 * node_scale >= 0 only on a stored node the program rescales; every index is dense and increasing; the counts and the
 * sentinel-ended tip edge list agree with the maps. */
static std::string check_storage_maps(int N, int E, const int *ip, const PlkProgram &pg, const PlkStorageMaps &m)
{
    if ((int)m.edge_tip.size() != E || (int)m.edge_int.size() != E || (int)m.node_int.size() != N || (int)m.node_scale.size() != N) return "storage maps: sizes";
    if (m.ntips != (int)pg.tip_edge.size() || (int)m.tip_edges.size() != m.ntips + 1 || m.tip_edges.back() != -1) return "storage maps: tip edge list";
    std::vector<int> slot_seen(m.ntips, 0);
    int nie = 0, nin = 0, nsc = 0, ntip = 0;
    for (int e = 0; e < E; e++) {
        if ((m.edge_tip[e] >= 0) == (m.edge_int[e] >= 0)) return "storage maps: edge " + std::to_string(e) + " is not exactly one of tip / internal";
        if (m.edge_tip[e] >= 0) {
            const int s = m.edge_tip[e];
            if (s >= m.ntips || slot_seen[s]++ || m.tip_edges[s] != e || pg.tip_edge[s] != e) return "storage maps: tip slot of edge " + std::to_string(e);
            ntip++;
        } else if (m.edge_int[e] != nie++) return "storage maps: edge_int is not dense and increasing";
    }
    if (ntip != m.ntips || nie != m.nie) return "storage maps: edge counts";
    for (int a = 0; a < N; a++) {
        const bool stored = ip[a + 1] > ip[a];
        if ((m.node_int[a] >= 0) != stored || m.node_int[a] < -1) return "storage maps: node_int of node " + std::to_string(a);
        if (stored && m.node_int[a] != nin++) return "storage maps: node_int is not dense and increasing";
        const bool scaled = stored && pg.scale_node[a];
        if ((m.node_scale[a] >= 0) != scaled || m.node_scale[a] < -1) return "storage maps: node_scale of node " + std::to_string(a);
        if (scaled && m.node_scale[a] != nsc++) return "storage maps: node_scale is not dense and increasing";
    }
    if (nin != m.nin || nsc != m.nsc) return "storage maps: node counts";
    return "";
}

static std::string check_tree(const Tree &t, const std::vector<char> &has, int nchar)
{
    const int N = t.N;
    PlkProgram pg;
    plk_program_build(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
    g_ops += (long)pg.ops.size();
    std::string bad = plk_program_check(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
    if (!bad.empty()) return bad;
    bad = check_scale_runs(t, has, pg);
    if (!bad.empty()) return bad;
    /* storage indices: the function the down / up drivers call, and its invariants; everything below runs on these maps */
    const int E = N - 1;
    PlkStorageMaps sm;
    plk_storage_maps_build(N, E, t.ip.data(), pg.tip_edge, pg.scale_node.data(), sm);
    bad = check_storage_maps(N, E, t.ip.data(), pg, sm);
    if (!bad.empty()) return bad;
    const std::vector<int> &edge_tip = sm.edge_tip, &edge_int = sm.edge_int, &node_int = sm.node_int, &node_scale = sm.node_scale;
    const int ntips = sm.ntips, nie = sm.nie, nin = sm.nin, nsc = sm.nsc;
    for (int mode = 0; mode <= 4; mode++) {
        PlkChain ch;
        if (mode == 4) {          /* mode 3 without node storage (the vector ll kernel) */
            plk_chain_build(N, pg, 3, t.ix.data(), nullptr, nullptr, nullptr, ch);
            bad = plk_chain_check(N, pg, ch, 3, 1 << 30, 0, 0, 0, 0, 0);
            if (!bad.empty()) return "mode 3 (ll): " + bad;
            continue;
        }
        plk_chain_build(N, pg, mode, t.ix.data(), node_int.data(), edge_int.data(), node_scale.data(), ch);
        const int block = mode == 1 ? 256 : 64;
        bad = plk_chain_check(N, pg, ch, mode, 1 << 30, nin, nie, nsc, block, pg.obs_nodes.size() * (size_t)block);
        if (!bad.empty()) return "mode " + std::to_string(mode) + ": " + bad;
        if (mode == 1 && !pg.ops.empty()) {      /* negative control: a broken chain link must be noticed */
            for (size_t pc = 0; pc < pg.ops.size(); pc++) {
                const int code = ch.ops[pc].x & 0xff;
                if (code == OP_TIP_SET || code == OP_TIP_MUL || code == OP_NODE_MUL) {
                    PlkChain c2 = ch;
                    c2.ops[pc].w += 1;
                    if (plk_chain_check(N, pg, c2, mode, 1 << 30, nin, nie, nsc, block, pg.obs_nodes.size() * (size_t)block).empty())
                        return "negative control: corrupted chain accepted";
                    break;
                }
            }
        }
    }
    /* visit records + matrix stream of the vector up pass, for every kind of query and with random masks */
    {
        std::vector<int> emask(E > 0 ? E : 1), nmask(N);
        unsigned lcg = 12345u + (unsigned)N * 7919u;
        for (int e = 0; e < E; e++) { lcg = lcg * 1664525u + 1013904223u; emask[e] = (lcg >> 24) % 3 != 0; }
        for (int a = 0; a < N; a++) { lcg = lcg * 1664525u + 1013904223u; nmask[a] = (lcg >> 24) % 3 != 0; }
        const int modes[3][2] = {{1, 0}, {0, 1}, {1, 1}};
        /* observed[a]: every site of leaf a is a single state (marginal queries then inline pre-terminal nodes too): none, a
         * pseudo-random half, all */
        std::vector<char> observed(N, 0);
        for (int md = 0; md < 3; md++)
            for (int masked = 0; masked < 2; masked++)
            for (int ob = 0; ob < (modes[md][1] ? 3 : 1); ob++) {
                for (int a = 0; a < N; a++) { lcg = lcg * 1664525u + 1013904223u; observed[a] = ob == 2 || (ob == 1 && (lcg >> 24) % 2); }
                PlkUpVisits uv;
                plk_up_visits_build(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), edge_tip.data(), node_int.data(),
                                    node_scale.data(), modes[md][0] != 0, modes[md][1] != 0, masked ? emask.data() : nullptr,
                                    masked ? nmask.data() : nullptr, uv, ob ? observed.data() : nullptr);
                bad = plk_up_visits_check(N, E, uv, nin, ntips, nsc, modes[md][0] != 0);
                if (!bad.empty()) return "up visits (deriv " + std::to_string(modes[md][0]) + ", marg " + std::to_string(modes[md][1]) + "): " + bad;
                if (modes[md][1]) {
                    /* every wanted marginal is produced exactly once: by a visit's child record, by the root's header, or by
                     * an inline record's leaf entry; an inlined node's leaves are all observed */
                    std::vector<int> mdone(N, 0);
                    size_t vp = 0;
                    for (int v = 0; v < uv.nvisits; v++) {
                        const int *h = &uv.rec[vp];
                        if (h[6]) mdone[h[0]]++;
                        for (int j = 0; j < h[1]; j++) {
                            const int *c = h + 8 + 4 * j;
                            if (c[2] & PLK_UP_WANT_M) mdone[c[0]]++;
                            if (c[2] & PLK_UP_INLINE) {
                                const int *q = &uv.rec[-2 - c[1]];
                                for (int l = 0; l < q[3]; l++) {
                                    if (q[7 + 3 * l] & 2) mdone[q[5 + 3 * l]]++;
                                    if (!ob || !observed[q[5 + 3 * l]]) return "up visits: a node with an unobserved leaf is inlined in a marginal pass";
                                }
                            }
                        }
                        vp += 8 + 4 * (size_t)h[1];
                    }
                    for (int a = 0; a < N; a++)
                        if (mdone[a] != ((!masked || nmask[a]) ? 1 : 0)) return "up visits: marginal of node " + std::to_string(a) + " produced " + std::to_string(mdone[a]) + " times";
                }
                if (md == 0 && !masked && !uv.kind.empty()) {      /* negative control: a dropped matrix must be noticed */
                    PlkUpVisits u2 = uv;
                    u2.kind.pop_back(); u2.edge.pop_back();
                    if (plk_up_visits_check(N, E, u2, nin, ntips, nsc, true).empty()) return "negative control: short matrix stream accepted";
                }
            }
    }
    /* node visits of the derivative up pass (k_up_nodes_mfma): every wanted edge is finished exactly once, and every
     * edge that is finished is wanted */
    if (E > 0) {
        std::vector<int> emask(E);
        unsigned lcg = 999u + (unsigned)N * 31u;
        for (int e = 0; e < E; e++) { lcg = lcg * 1664525u + 1013904223u; emask[e] = (lcg >> 24) % 4 == 0; }
        for (int masked = 0; masked < 2; masked++) {
            PlkUpNodes un;
            plk_up_nodes_build(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), edge_tip.data(), node_int.data(),
                               node_scale.data(), masked ? emask.data() : nullptr, un);
            bad = plk_up_nodes_check(N, E, t.ip.data(), t.ix.data(), un, nin, ntips, nsc);
            if (!bad.empty()) return std::string("up nodes (") + (masked ? "masked" : "all edges") + "): " + bad;
            std::vector<int> done(E, 0);
            size_t vp = 0;
            for (int v = 0; v < un.nvisits; v++) {
                const int *h = &un.rec[vp];
                if ((h[7] & PLK_UN_OWN_D) && h[6] >= 0) done[h[6]]++;
                for (int j = 0; j < h[1]; j++) if (h[8 + 4 * j + 2] & PLK_UN_LEAF_D) done[h[5] + (h[8 + 4 * j + 2] >> PLK_UN_POS_SHIFT)]++;
                vp += 8 + 4 * (size_t)h[1];
            }
            for (int e = 0; e < E; e++)
                if (done[e] != ((!masked || emask[e]) ? 1 : 0)) return "up nodes: edge " + std::to_string(e) + " finished " + std::to_string(done[e]) + " times";
            if (!masked) {                 /* negative control: drop the first stored vector, its reader must be caught */
                PlkUpNodes u2 = un;
                for (size_t q = 0, w = 0; w < (size_t)u2.nvisits; w++) {
                    const int dg = u2.rec[q + 1];
                    bool hit = false;
                    for (int j = 0; j < dg; j++) if (u2.rec[q + 8 + 4 * j + 2] & PLK_UN_STORE_G) { u2.rec[q + 8 + 4 * j + 2] &= ~PLK_UN_STORE_G; hit = true; break; }
                    if (hit) { if (plk_up_nodes_check(N, E, t.ip.data(), t.ix.data(), u2, nin, ntips, nsc).empty()) return "negative control: unwritten vector accepted (up nodes)"; break; }
                    q += 8 + 4 * (size_t)dg;
                }
            }
        }
    }
    /* the k = 4 node visits with pair tables and table-rebuilt children (run_updown4): pair nodes as the engine picks them,
     * rebuild table, records, and a negative control (an entry that names the wrong table must be refused) */
    if (E > 0) {
        std::vector<int> pair_of(N, -1), edge_into(N, -1);
        for (int a = 0; a < N; a++) for (int idx = t.ip[a]; idx < t.ip[a + 1]; idx++) edge_into[t.ix[idx]] = idx;
        int npairs = 0;
        for (int b = 0; b < N; b++) {
            const int e0 = t.ip[b];
            if (t.ip[b + 1] - e0 != 2 || edge_into[b] < 0 || has[b]) continue;
            if (edge_tip[e0] < 0 || edge_tip[e0 + 1] < 0) continue;
            pair_of[b] = npairs++;
        }
        std::vector<char> rb;
        std::vector<int> rtab;
        plk_up_rebuild_table(N, t.ip.data(), t.ix.data(), has.data(), edge_tip.data(), node_int.data(), node_scale.data(), pair_of.data(), nin, rb, rtab);
        PlkUpNodes un;
        plk_up_nodes_build(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), edge_tip.data(), node_int.data(), node_scale.data(), nullptr, un,
                           pair_of.data(), rb.data());
        bad = plk_up_nodes_check(N, E, t.ip.data(), t.ix.data(), un, nin, ntips, nsc, npairs, edge_tip.data(), rtab.data(), pair_of.data());
        if (!bad.empty()) return "up nodes (pairs, rebuilt children): " + bad;
        /* pair children finished inside their parent's visit, without and with an edge mask: every wanted edge still exactly once */
        {
            std::vector<int> emask(E);
            unsigned lcg2 = 4242u + (unsigned)N * 17u;
            for (int e = 0; e < E; e++) { lcg2 = lcg2 * 1664525u + 1013904223u; emask[e] = (lcg2 >> 24) % 3 != 0; }
            for (int masked = 0; masked < 2; masked++) {
                PlkUpNodes ui;
                plk_up_nodes_build(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), edge_tip.data(), node_int.data(), node_scale.data(),
                                   masked ? emask.data() : nullptr, ui, pair_of.data(), rb.data(), true);
                bad = plk_up_nodes_check(N, E, t.ip.data(), t.ix.data(), ui, nin, ntips, nsc, npairs, edge_tip.data(), rtab.data(), pair_of.data());
                if (!bad.empty()) return "up nodes (inline pair children): " + bad;
                std::vector<int> done(E, 0);
                size_t vq = 0;
                for (int v = 0; v < ui.nvisits; v++) {
                    const int *h = &ui.rec[vq];
                    if ((h[7] & PLK_UN_OWN_D) && h[6] >= 0) done[h[6]]++;
                    for (int j = 0; j < h[1]; j++) {
                        const int fl = h[8 + 4 * j + 2], b = h[8 + 4 * j];
                        if (fl & PLK_UN_LEAF_D) done[h[5] + (fl >> PLK_UN_POS_SHIFT)]++;
                        if (fl & PLK_UN_INL_OWN) done[h[5] + (fl >> PLK_UN_POS_SHIFT)]++;
                        if (fl & PLK_UN_INL_L0) done[t.ip[b]]++;
                        if (fl & PLK_UN_INL_L1) done[t.ip[b] + 1]++;
                        if ((fl & PLK_UN_INL) && h[1] > 2) return "up nodes: inline pair child under a node with more than two children";
                    }
                    vq += 8 + 4 * (size_t)h[1];
                }
                for (int e = 0; e < E; e++)
                    if (done[e] != ((!masked || emask[e]) ? 1 : 0)) return "up nodes (inline pairs): edge " + std::to_string(e) + " finished " + std::to_string(done[e]) + " times";
            }
        }
        int nflag = 0, nrb = 0;
        size_t vp = 0;
        for (int v = 0; v < un.nvisits; v++) {
            const int *h = &un.rec[vp];
            for (int j = 0; j < h[1]; j++) if (h[8 + 4 * j + 2] & PLK_UN_REBUILD) nflag++;
            vp += 8 + 4 * (size_t)h[1];
        }
        for (int b = 0; b < N; b++) if (rb[b]) {
            nrb++;
            if (pair_of[b] >= 0 || has[b] || t.ip[b + 1] - t.ip[b] != 2) return "rebuild table: node " + std::to_string(b) + " does not qualify";
        }
        if (nflag != nrb) return "up nodes: " + std::to_string(nrb) + " rebuilt nodes, " + std::to_string(nflag) + " flagged child records";
        if (nrb > 0) {
            std::vector<int> r2 = rtab;
            for (int b = 0; b < N; b++) if (rb[b]) { r2[4 * (size_t)node_int[b]] += r2[4 * (size_t)node_int[b]] >= 0 ? 1 : -1; break; }
            if (plk_up_nodes_check(N, E, t.ip.data(), t.ix.data(), un, nin, ntips, nsc, npairs, edge_tip.data(), r2.data(), pair_of.data()).empty())
                return "negative control: rebuild entry with the wrong table accepted";
        }
    }
    if (pg.slots_needed > PLK_FUSED_SLOTS) return "";
    PlkFused fu;
    plk_fused_build(N, pg, fu);
    for (int NS = 1; NS <= 2; NS++) {
        const size_t lds = plk_fused_lds_bytes(pg, nchar, PLK_TILE * NS);
        if (lds > PLK_LDS_LIMIT || (NS == 2 && pg.slots_needed > 8)) continue;
        const int D = pg.slots_needed <= 4 ? 4 : (pg.slots_needed <= 8 ? 8 : 16);
        bad = plk_fused_check_cpp(N, pg, fu, nchar, D, NS, lds);
        if (!bad.empty()) return "NS " + std::to_string(NS) + ": " + bad;
    }
    if (fu.asm_ok) {
        for (int pack4 = 0; pack4 <= 1; pack4++) {
            if (pack4 && nchar > 16) continue;
            const size_t lds = plk_fused_lds_bytes(pg, nchar, pack4 ? PLK_TILE / 2 : PLK_TILE);
            if (lds > PLK_LDS_LIMIT) continue;
            const int D = pg.slots_needed <= 4 ? 4 : 8;
            bad = plk_fused_check_asm(N, pg, fu, nchar, D, pack4, lds);
            if (!bad.empty()) return "pack4 " + std::to_string(pack4) + ": " + bad;
            /* negative controls: one byte less of LDS, a field pushed out of range, a lost END */
            if (plk_fused_check_asm(N, pg, fu, nchar, D, pack4, lds - 1).empty()) return "negative control: short LDS accepted";
            PlkFused f2 = fu;
            bool touched = false;
            for (size_t w = 0; w < f2.words.size() && !touched; w++)
                if ((f2.words[w] & 31) <= 1) { f2.words[w] = (f2.words[w] & 0xffff) | ((unsigned)pg.obs_nodes.size() << 16); touched = true; }
            if (touched && plk_fused_check_asm(N, pg, f2, nchar, D, pack4, lds).empty()) return "negative control: row field out of range accepted";
            f2 = fu;
            for (size_t w = 0; w < f2.words.size(); w++)
                if ((f2.words[w] & 31) == OP_END) { f2.words[w] = OP_SCALE; break; }      /* the first END overwritten */
            if (plk_fused_check_asm(N, pg, f2, nchar, D, pack4, lds).empty()) return "negative control: missing END accepted";
        }
    }
    /* the vector ll kernel's program on pair tables (any stack depth, any nchar): every cherry, a budget of two */
    if (!pg.obs_nodes.empty()) {
        const int vbud[2] = {1 << 30, 2};
        for (int bi = 0; bi < 2; bi++) {
            PlkFusedPT fp;
            plk_fused_pt_build(N, t.ip.data(), t.ix.data(), pg, nchar, vbud[bi], fp, false);
            PlkVecPT vp;
            plk_vec_pt_build(fp, nchar, vp);
            bad = plk_vec_pt_check(N, t.ip.data(), t.ix.data(), pg, fp, vp, nchar, E);
            if (!bad.empty()) return "vec pt budget " + std::to_string(bi) + ": " + bad;
            if (bi == 0 && fp.npairs > 0) {           /* negative controls */
                PlkVecPT v2 = vp;
                for (size_t q = 0; q < v2.ops.size(); q++) if ((v2.ops[q].x & 0xff) == OP_TIP_SET) { v2.ops[q].y += nchar; break; }
                if (plk_vec_pt_check(N, t.ip.data(), t.ix.data(), pg, fp, v2, nchar, E).empty()) return "negative control (vec pt): shifted table accepted";
                v2 = vp;
                bool changed = false;
                for (size_t q = 0; q < v2.op_edge.size() && !changed; q++) if (v2.op_edge[q] >= 0) { v2.op_edge[q] = (v2.op_edge[q] + 1) % (E > 0 ? E : 1); changed = true; }
                if (changed && E > 1 && plk_vec_pt_check(N, t.ip.data(), t.ix.data(), pg, fp, v2, nchar, E).empty()) return "negative control (vec pt): wrong matrix accepted";
            }
        }
    }
    /* pair-table interpreter (k_ll_fused4_asm_pt): with every cherry as a table, with a budget of one, with none */
    if (pg.slots_needed <= 4 && nchar <= 16 && !pg.obs_nodes.empty()) {
        const int budgets[3] = {1 << 30, 1, 0};
        for (int bi = 0; bi < 3; bi++) {
            PlkFusedPT fp;
            plk_fused_pt_build(N, t.ip.data(), t.ix.data(), pg, nchar, budgets[bi], fp);
            if (fp.npairs > budgets[bi]) return "pt: more pair tables than the budget";
            const int tile = (N + bi) % 2 ? 512 : 1024;
            const size_t lds = plk_fused_pt_lds_bytes(fp, nchar, tile);
            if (lds > plk_pt_lds_limit(tile) || fp.units >= 2048) continue;
            bad = plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, fp, nchar, tile, lds);
            if (!bad.empty()) return "pt budget " + std::to_string(bi) + ": " + bad;
            /* every edge is either a matrix of the stream, the leaf edge of a one-unit table, or one of the three edges
             * of a pair table -- exactly once */
            std::vector<int> seen(E > 0 ? E : 1, 0);
            for (int e : fp.mat_edge) seen[e]++;
            for (size_t q = 0; q < fp.tab_edge.size(); q++) {
                if (fp.tab_edge[q] >= 0) seen[fp.tab_edge[q]]++;
                if (fp.tab_eb[q] >= 0) { seen[fp.tab_eb[q]]++; seen[fp.tab_ec[q]]++; }
            }
            for (int e = 0; e < E; e++) if (seen[e] != 1) return "pt: edge " + std::to_string(e) + " covered " + std::to_string(seen[e]) + " times";
            {
                /* the two-sites-per-lane interpreter's words: TIP_SET + POPMUL / PUSH fused, re-encoded as 64-bit ops */
                PlkFusedPT fq;
                plk_fused_pt_build(N, t.ip.data(), t.ix.data(), pg, nchar, budgets[bi], fq, true);
                const int tile4 = (N + bi) % 2 ? 1024 : 1536;
                const size_t lds4 = plk_fused_pt_lds_bytes(fq, nchar, tile4);
                if (lds4 <= plk_pt_lds_limit(tile4) && fq.units < 2048) {
                    bad = plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, fq, nchar, tile4, lds4, true);
                    if (!bad.empty()) return "v4 words, budget " + std::to_string(bi) + ": " + bad;
                    if (fq.words != fp.words && plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, fq, nchar, tile4, lds4, false).empty())
                        return "negative control (v4): fused SET words accepted by the one-site interpreter's check";
                    PlkFusedV4 v4;
                    plk_fused_v4_words(fq, nchar, tile4, 256, v4);
                    bad = plk_fused_check_v4(fq, v4, nchar, tile4, 256, lds4);
                    if (!bad.empty()) return "v4 encoding: " + bad;
                    PlkFusedV4 v5 = v4;
                    v5.words[1] += 1u << 16;
                    if (plk_fused_check_v4(fq, v5, nchar, tile4, 256, lds4).empty() && plk_word_is_obs(fq.words[0] & 31)) return "negative control (v4): shifted table offset accepted";
                }
            }
            if (bi != 0) continue;
            /* negative controls */
            if (plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, fp, nchar, tile, lds - 1).empty()) return "negative control (pt): short LDS accepted";
            PlkFusedPT f2 = fp;
            for (size_t w = 0; w < f2.words.size(); w++)
                if ((f2.words[w] & 31) == OP_END) { f2.words[w] = OP_SCALE; break; }
            if (plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, f2, nchar, tile, lds).empty()) return "negative control (pt): missing END accepted";
            if (fp.npairs > 0) {
                f2 = fp;
                for (size_t q = 0; q < f2.tab_eb.size(); q++) if (f2.tab_eb[q] >= 0) { std::swap(f2.tab_eb[q], f2.tab_edge[q]); break; }
                if (plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, f2, nchar, tile, lds).empty()) return "negative control (pt): pair table with swapped edges accepted";
                f2 = fp;
                for (size_t r = 0; r < f2.row_node2.size(); r++) if (f2.row_node2[r] >= 0) { f2.row_node2[r] = -1; break; }
                if (plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, f2, nchar, tile, lds).empty()) return "negative control (pt): pair row without its second node accepted";
            }
            f2 = fp;
            bool touched = false;
            for (size_t w = 0; w < f2.words.size() && !touched; w++)
                if ((f2.words[w] & 31) <= 1) { f2.words[w] = (f2.words[w] & 0xffff) | ((unsigned)fp.row_node.size() << 16); touched = true; }
            if (touched && plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, f2, nchar, tile, lds).empty()) return "negative control (pt): row field out of range accepted";
        }
    }
    return "";
}

/* The site-chunk rules as the down / up drivers spelled them inline before plk_site_chunk() existed: the reference of the
 * table below.  Ordinary rule (run_updown4, run_updown_vec, run_updown, second_order_generic, second_order_k4), 0 where
 * they reported "not enough device memory for one site": */
static long ref_chunk_ordinary(long S, size_t free_b, size_t work_bytes, size_t per_site, long opt_site_chunk, int BLOCK)
{
    size_t budget = free_b > (size_t)(6ull << 30) ? free_b - (size_t)(4ull << 30) : free_b / 2;
    budget += work_bytes;
    long chunk = (long)std::min<size_t>((size_t)S, budget / per_site);
    if (opt_site_chunk > 0) chunk = std::min<long>(chunk, opt_site_chunk);
    if (chunk < 1) return 0;
    if (chunk < S) chunk = std::max<long>(BLOCK, chunk / BLOCK * BLOCK);
    return chunk;
}
/* ... and the matrix-core rule (run_updown_mfma), 0 where it reported "not enough device memory" */
static long ref_chunk_mfma(long S, size_t free_b, size_t work_bytes, size_t per_site, long opt_site_chunk, int MF_SITES)
{
    size_t budget = free_b > (size_t)(6ull << 30) ? free_b - (size_t)(4ull << 30) : free_b / 2;
    budget += work_bytes;
    long chunk = (long)std::min<size_t>((size_t)((S + MF_SITES - 1) / MF_SITES * MF_SITES), budget / per_site);
    if (opt_site_chunk > 0) chunk = std::min<long>(chunk, opt_site_chunk);
    chunk = chunk / MF_SITES * MF_SITES;
    if (chunk < MF_SITES) return 0;
    return chunk;
}

static std::string check_chunk_planner()
{
    const size_t GiB = (size_t)1 << 30, MiB = (size_t)1 << 20;
    const int tiles[3] = {64, 128, 256};
    struct Case { long S_tiles, S_extra; size_t free_b, work_b, per_site; long opt_num, opt_den; const char *what; };
    /* S = S_tiles * tile + S_extra, opt_site_chunk = tile * opt_num / opt_den */
    const Case cases[] = {
        {0, -1, 64 * GiB, 0, 1000, 0, 1, "S below one tile"},                      /* S_extra -1: tile - 1 sites */
        {4, 0, 64 * GiB, 0, 1000, 0, 1, "S a whole number of tiles"},
        {4, 1, 64 * GiB, 0, 1000, 0, 1, "S one over"},
        {4, 1, 64 * GiB, 0, 1000, 2, 1, "forced chunk of two tiles"},
        {4, 1, 64 * GiB, 0, 1000, 5, 2, "forced chunk of two and a half tiles"},
        {10, 0, 64 * GiB, 0, 1000, 1, 2, "forced chunk below the tile"},           /* ordinary: one tile; matrix core: does not fit */
        {0, -1, 64 * GiB, 0, 1000, 1, 2, "forced chunk below the tile, S below the tile"},
        {10, 0, 2 * 1000 - 2, 0, 1000, 0, 1, "budget just below one site"},
        {10, 0, 2 * 1000, 0, 1000, 0, 1, "budget of exactly one site"},            /* ordinary: rounded up to one tile */
        {10, 0, 2 * 1000 - 2, 1, 1000, 0, 1, "the retained workspace makes one site fit"},
        {10, 0, 0, 0, 1000, 0, 1, "no memory at all"},
        {1000, 0, 6 * GiB, 0, MiB, 0, 1, "6 GiB free: half of it"},
        {1000, 0, 6 * GiB + MiB, 0, MiB, 0, 1, "just above 6 GiB free: all but 4 GiB"},
        {1000, 0, 6 * GiB, GiB, MiB, 0, 1, "retained workspace added after the 6 GiB branch"},
        {1000, 0, 5 * GiB + MiB, GiB, MiB, 0, 1, "retained workspace does not move the branch"},
        {1000, 3, 64 * GiB, 0, 16 * MiB, 0, 1, "memory-bound chunk, ragged S"},
    };
    for (int ti = 0; ti < 3; ti++)
        for (const Case &c : cases) {
            const int tile = tiles[ti];
            const long S = c.S_tiles * tile + (c.S_extra < 0 ? tile + c.S_extra : c.S_extra), opt = tile * c.opt_num / c.opt_den;
            for (int mc = 0; mc < 2; mc++) {
                const long want = mc ? ref_chunk_mfma(S, c.free_b, c.work_b, c.per_site, opt, tile) : ref_chunk_ordinary(S, c.free_b, c.work_b, c.per_site, opt, tile);
                const long got = plk_site_chunk(S, c.free_b, c.work_b, c.per_site, opt, tile, mc != 0);
                if (got != want)
                    return std::string("chunk planner (") + c.what + ", tile " + std::to_string(tile) + (mc ? ", matrix-core rule): " : ", ordinary rule): ") +
                           std::to_string(got) + ", the inline formula gives " + std::to_string(want);
            }
        }
    /* a few values worked out by hand, so that the reference is pinned too (tile 64, 1 MiB per site, 64000 sites) */
    struct Lit { size_t free_b, work_b; long opt; bool mc; long want; };
    const Lit lits[] = {
        {6 * GiB, 0, 0, false, 3072}, {6 * GiB + MiB, 0, 0, false, 2048}, {6 * GiB, GiB, 0, false, 4096}, {6 * GiB + MiB, 0, 0, true, 2048},
        {64 * GiB, 0, 32, false, 64}, {64 * GiB, 0, 32, true, 0}, {2 * MiB, 0, 0, false, 64}, {2 * MiB, 0, 0, true, 0}, {2 * MiB - 2, 0, 0, false, 0},
        {64 * GiB, 0, 0, false, 61440}, {64 * GiB, 0, 100000, true, 61440},
    };
    for (const Lit &l : lits) {
        const long got = plk_site_chunk(64000, l.free_b, l.work_b, MiB, l.opt, 64, l.mc);
        if (got != l.want) return "chunk planner: literal case gives " + std::to_string(got) + ", expected " + std::to_string(l.want);
    }
    return "";
}

/* ------------------------------------------------------------------------------------------------------------ */
/* which k = 4 ll kernel runs (plk_k4_choose): the choice pinned on the CPU                                       */
/* ------------------------------------------------------------------------------------------------------------ */

/* static LDS of k_ll_fused4_v4s<768>, k_ll_fused4_v4<768>, k_ll_fused4_v4<512> as compiled for gfx950 (the engine asks the runtime) */
static const size_t K4_STATIC_LDS[3] = {0, 256, 256};

enum { OUT_CPP_D4, OUT_CPP_D8, OUT_CPP_D16, OUT_CPP_NS2, OUT_ASM_D4_P0, OUT_ASM_D4_P1, OUT_ASM_D8_P0, OUT_ASM_D8_P1, OUT_PT_512, OUT_PT_1024,
       OUT_V4_1024, OUT_V4_1536, OUT_V4S, OUT_NONE, OUT_COUNT };
static const char *const OUT_NAME[OUT_COUNT] = {"C++ NS 1 D 4", "C++ NS 1 D 8", "C++ NS 1 D 16", "C++ NS 2", "asm D 4 pack4 0", "asm D 4 pack4 1",
    "asm D 8 pack4 0", "asm D 8 pack4 1", "asm_pt 512", "asm_pt 1024", "v4 1024", "v4 1536", "v4s", "not fused"};
static long g_outcome[OUT_COUNT];
/* per PLK_OPT_PAIR_TABLES mode: cases in which a forced mode's own tile kernel did not fit while another tile kernel would
 * have -- the cases that tell "falls through to the interpreters" from "falls back to another pair-table candidate" */
static long g_forced_fell_through[8];

struct K4Formats { PlkFused fu; PlkFusedPT fpt; PlkFusedV4 fv4; PlkFusedV4S fv4s; };
struct K4Cand { PlkK4Variant variant; int tile; };

static bool pt_fields_ok(const PlkFusedPT &f) { return f.units < 2048 && f.row_node.size() < 65536; }

/* Does a tile candidate fit with some number of cherries as tables?  A cherry as a table adds a fixed number of bytes
 * (of either sign) to the image, so the smallest image has every cherry or none: both ends are tried. */
static bool pt_cand_fits(const Tree &t, const PlkProgram &pg, int nchar, const K4Cand &cd)
{
    const int budgets[2] = {INT_MAX, 0};
    for (int b = 0; b < 2; b++) {
        PlkFusedPT f;
        plk_fused_pt_build(t.N, t.ip.data(), t.ix.data(), pg, nchar, budgets[b], f, cd.variant == PLK_K4_V4);
        if (plk_fused_pt_lds_bytes(f, nchar, cd.tile) <= plk_pt_lds_limit(cd.tile) && pt_fields_ok(f)) return true;
    }
    return false;
}

static bool stream_fits(const Tree &t, const PlkProgram &pg, int nchar, int C)
{
    PlkFusedPT f;
    plk_fused_pt_build(t.N, t.ip.data(), t.ix.data(), pg, nchar, INT_MAX, f, true);
    bool any_obs = false;
    for (const PlkFusedPT::VOp &o : f.vops) any_obs = any_obs || o.code == OP_TIP_SET || o.code == OP_TIP_MUL;
    const size_t image = K4_STATIC_LDS[PLK_K4_LDS_V4S_768] + plk_fused_v4s_lds_bytes(f, nchar, C);
    return any_obs && image <= plk_pt_lds_limit(1024) && image / 32 < 65536 && pt_fields_ok(f);
}

static PlkK4Choice k4_choose(const Tree &t, const PlkProgram &pg, int nchar, int C, long S, long mode, long fasm, long spl, bool allow_stream, K4Formats &F)
{
    PlkK4Shape sh = {nchar, C, S, 256, mode, fasm, spl, {K4_STATIC_LDS[0], K4_STATIC_LDS[1], K4_STATIC_LDS[2]}};
    return plk_k4_choose(t.N, t.ip.data(), t.ix.data(), pg, sh, allow_stream, F.fu, F.fpt, F.fv4, F.fv4s);
}

/* One tree through the sweep of nchar, C, S, PLK_OPT_PAIR_TABLES, PLK_OPT_FUSED_ASM, PLK_OPT_FUSED_SITES_PER_LANE and
 * allow_stream (256 CUs).  For every case: the candidates in the engine's order of preference are written out here, each
 * with its own fit test from the *_lds_bytes functions; the choice must be the first that fits (so no earlier one would
 * have fitted, and a forced mode gives its kernel and tile or falls through to the interpreters); the chosen variant's
 * preconditions hold and its replay check, run again here on the formats handed back, is empty. */
static std::string check_k4_choice(const Tree &t, const std::vector<char> &has, const int *nchars, int n_nchars)
{
    const int N = t.N;
    const int *ip = t.ip.data(), *ix = t.ix.data();
    PlkProgram pg;
    plk_program_build(N, ip, ix, t.pre.data(), has.data(), pg);
    const int slots = pg.slots_needed;
    const K4Cand tiles[4] = {{PLK_K4_V4, 1536}, {PLK_K4_V4, 1024}, {PLK_K4_ASM_PT, 1024}, {PLK_K4_ASM_PT, 512}};
    const long modes[7] = {0, 1, 2, 3, 5, 6, 7}, sites[4] = {1, 300, 1250000, 10000000};
    for (int ni = 0; ni < n_nchars; ni++) {
        const int nchar = nchars[ni];
        const bool pt_tree = slots <= 4 && nchar <= 16 && !pg.obs_nodes.empty();
        bool tile_fits[4] = {false, false, false, false};
        for (int q = 0; q < 4 && pt_tree; q++) tile_fits[q] = pt_cand_fits(t, pg, nchar, tiles[q]);
        for (int C = 1; C <= 4; C += 3) {
            const bool sfits = pt_tree && stream_fits(t, pg, nchar, C);
            for (long S : sites) for (long mode : modes) for (long fasm = 0; fasm <= 1; fasm++) for (long spl = 0; spl <= 2; spl += 2)
            for (int allow = 0; allow <= 1; allow++) {
                const std::string tag = plk_fmt("k4 choice (nchar %ld, C %ld, ", nchar, C) + plk_fmt("S %ld, mode %ld, asm %ld, ", S, mode, fasm) +
                                        plk_fmt("sites per lane %ld, stream %ld): ", spl, allow);
                K4Formats F;
                const PlkK4Choice ch = k4_choose(t, pg, nchar, C, S, mode, fasm, spl, allow != 0, F);
                /* the interpreters */
                const int NS = spl == 2 && slots <= 8 ? 2 : 1, pack4 = nchar <= 16 ? 1 : 0;
                const size_t lds_cpp = plk_fused_lds_bytes(pg, nchar, PLK_TILE * NS), lds_asm = plk_fused_lds_bytes(pg, nchar, pack4 ? PLK_TILE / 2 : PLK_TILE);
                const bool asm_fits = NS == 1 && fasm && plk_fused_asm_ok(pg) && lds_asm <= PLK_LDS_LIMIT;
                const bool fused = slots <= PLK_FUSED_SLOTS && (asm_fits || lds_cpp <= PLK_LDS_LIMIT);
                /* the order of preference, with what fits */
                std::vector<K4Cand> order;
                std::vector<char> fits;
                if (fused && pt_tree && mode != 0 && fasm && spl != 2) {
                    if ((mode == 1 || mode == 7) && allow) { order.push_back({PLK_K4_V4S, 1536}); fits.push_back(sfits); }
                    int pick[4] = {0, 1, 2, 3}, npick = 4;
                    if (mode == 2) { pick[0] = 2; npick = 1; }
                    else if (mode == 3) { pick[0] = 3; npick = 1; }
                    else if (mode == 5) { pick[0] = 1; npick = 1; }
                    else if (mode == 6) { pick[0] = 0; npick = 1; }
                    else {
                        /* 1024-site tiles first when their rounds over 256 CUs cost less than 1.3 x those of 1536-site tiles */
                        const long r1024 = ((S + 1023) / 1024 + 255) / 256, r1536 = ((S + 1535) / 1536 + 255) / 256;
                        if (10 * r1024 < 13 * r1536) std::swap(pick[0], pick[1]);
                    }
                    for (int q = 0; q < npick; q++) { order.push_back(tiles[pick[q]]); fits.push_back(tile_fits[pick[q]]); }
                }
                if (fused) { order.push_back(asm_fits ? K4Cand{PLK_K4_ASM, PLK_TILE} : K4Cand{PLK_K4_CPP, PLK_TILE * NS}); fits.push_back(1); }
                order.push_back({PLK_K4_NONE, 0}); fits.push_back(1);
                size_t first = 0;
                while (!fits[first]) first++;
                if (ch.variant != order[first].variant || ch.tile != order[first].tile)
                    return tag + plk_fmt("variant %ld at tile %ld chosen, ", ch.variant, ch.tile) + plk_fmt("the order of preference gives variant %ld at tile %ld", order[first].variant, order[first].tile);
                if (mode == 2 || mode == 3 || mode == 5 || mode == 6) {
                    const K4Cand forced = tiles[mode == 2 ? 2 : mode == 3 ? 3 : mode == 5 ? 1 : 0];
                    const bool pt_variant = ch.variant == PLK_K4_ASM_PT || ch.variant == PLK_K4_V4 || ch.variant == PLK_K4_V4S;
                    if (pt_variant && (ch.variant != forced.variant || ch.tile != forced.tile)) return tag + "a forced mode ran another pair-table kernel";
                    if (order.size() > 2 && !fits[0] && (tile_fits[0] || tile_fits[1] || tile_fits[2] || tile_fits[3])) g_forced_fell_through[mode]++;
                }
                if (!ch.bad.empty()) return tag + ch.bad;
                /* preconditions and replay of the chosen variant, from the formats handed back */
                std::string bad;
                int out = OUT_NONE;
                if (ch.variant == PLK_K4_CPP) {
                    const int D = slots <= 4 ? 4 : slots <= 8 ? 8 : 16;
                    if (ch.D != D || ch.NS != NS || ch.block != PLK_TILE || ch.lds != lds_cpp || lds_cpp > PLK_LDS_LIMIT || (NS == 2 && (spl != 2 || slots > 8))) return tag + "C++ interpreter: preconditions";
                    bad = plk_fused_check_cpp(N, pg, F.fu, nchar, D, NS, lds_cpp);
                    out = NS == 2 ? OUT_CPP_NS2 : D == 4 ? OUT_CPP_D4 : D == 8 ? OUT_CPP_D8 : OUT_CPP_D16;
                } else if (ch.variant == PLK_K4_ASM) {
                    const int D = slots <= 4 ? 4 : 8;
                    if (ch.D != D || ch.NS != 1 || ch.pack4 != pack4 || ch.block != PLK_TILE || ch.lds != lds_asm || lds_asm > PLK_LDS_LIMIT || slots > 8 || !fasm || (spl == 2 && slots <= 8))
                        return tag + "assembly interpreter: preconditions";
                    bad = plk_fused_check_asm(N, pg, F.fu, nchar, D, pack4, lds_asm);
                    out = (D == 4 ? OUT_ASM_D4_P0 : OUT_ASM_D8_P0) + pack4;
                } else if (ch.variant == PLK_K4_ASM_PT || ch.variant == PLK_K4_V4) {
                    const bool v4 = ch.variant == PLK_K4_V4;
                    const size_t lds = plk_fused_pt_lds_bytes(F.fpt, nchar, ch.tile);
                    if (slots > 4 || nchar > 16 || !fasm || spl == 2 || mode == 0 || !plk_pt_tile_ok(ch.tile) || (v4 ? ch.tile == 512 : ch.tile == 1536) || ch.lds != lds ||
                        lds > plk_pt_lds_limit(ch.tile) || !pt_fields_ok(F.fpt) || ch.block != (v4 ? ch.tile / 2 : ch.tile) || ch.NS != (v4 ? 2 : 1) || ch.D != 4) return tag + "pair-table tile kernel: preconditions";
                    bad = plk_fused_check_pt(N, ip, ix, pg, F.fpt, nchar, ch.tile, lds, v4);
                    if (v4) {
                        const unsigned base = (unsigned)K4_STATIC_LDS[ch.tile == 1536 ? PLK_K4_LDS_V4_768 : PLK_K4_LDS_V4_512];
                        if (ch.tip_base != base) return tag + "v4: table base";
                        if (bad.empty()) bad = plk_fused_check_v4(F.fpt, F.fv4, nchar, ch.tile, base, lds);
                    }
                    out = v4 ? (ch.tile == 1024 ? OUT_V4_1024 : OUT_V4_1536) : (ch.tile == 512 ? OUT_PT_512 : OUT_PT_1024);
                } else if (ch.variant == PLK_K4_V4S) {
                    const size_t lds = plk_fused_v4s_lds_bytes(F.fpt, nchar, C), st = K4_STATIC_LDS[PLK_K4_LDS_V4S_768];
                    if (slots > 4 || nchar > 16 || !fasm || spl == 2 || (mode != 1 && mode != 7) || !allow || S < 1 || ch.lds != lds || ch.tip_base != st ||
                        lds + st > plk_pt_lds_limit(1024) || !pt_fields_ok(F.fpt) || ch.block != 768 || ch.tile != 1536 || F.fpt.npairs < 0) return tag + "streamed form: preconditions";
                    bad = plk_fused_check_pt(N, ip, ix, pg, F.fpt, nchar, 1, 0, true, false);
                    if (bad.empty()) bad = plk_fused_check_v4s(F.fpt, F.fv4s, nchar, C, (unsigned)st, lds);
                } else if (slots <= PLK_FUSED_SLOTS && (lds_cpp <= PLK_LDS_LIMIT || asm_fits)) return tag + "not fused although an interpreter fits";
                if (ch.variant == PLK_K4_V4S) out = OUT_V4S;
                if (!bad.empty()) return tag + "replay: " + bad;
                g_outcome[out]++;
            }
        }
    }
    return "";
}

static bool tree_from_parents(const std::vector<int> &parent, Tree &t)       /* parent[i] of node i >= 1, node 0 the root */
{
    const int N = (int)parent.size();
    std::vector<int> ea(N - 1), eb(N - 1);
    for (int i = 1; i < N; i++) { ea[i - 1] = parent[i]; eb[i - 1] = i; }
    return make_tree(N, ea, eb, t);
}

/* n leaves, one joining per level (nodes: 0 the root, odd i a leaf under i - 1 or, the last two, the cherry) */
static void caterpillar_tree(int n, Tree &t)
{
    std::vector<int> parent(2 * n - 1, 0);
    for (int i = 1; i < 2 * n - 1; i++) parent[i] = i % 2 ? i - 1 : i - 2;
    tree_from_parents(parent, t);
}

static void balanced_tree(int leaves, Tree &t)
{
    std::vector<int> parent(2 * leaves - 1, 0);
    for (int i = 1; i < 2 * leaves - 1; i++) parent[i] = (i - 1) / 2;
    tree_from_parents(parent, t);
}

/* the irregular tree of the GPU tests' k = 4 models "irregular" and "wide" (tests/helpers.py), with data on nodes 17 and 18 */
static void irregular_tree(Tree &t, std::vector<char> &has)
{
    const int e[23][2] = {{13, 14}, {13, 15}, {13, 12}, {14, 16}, {14, 4}, {14, 5}, {16, 6}, {16, 17}, {17, 7}, {17, 18}, {18, 2}, {18, 3},
                          {15, 19}, {19, 8}, {19, 20}, {20, 9}, {20, 21}, {21, 10}, {21, 22}, {22, 11}, {22, 23}, {23, 0}, {23, 1}};
    std::vector<int> ea(23), eb(23);
    for (int i = 0; i < 23; i++) { ea[i] = e[i][0]; eb[i] = e[i][1]; }
    make_tree(24, ea, eb, t);
    has.assign(24, 0);
    has[17] = has[18] = 1;
}

/* (shape, options) -> (PLK_INFO_LL_KERNEL is 1 throughout) variant, form, sites per tile: the shapes of the GPU tests
 * test_gpu_k4_variants.py, test_gpu_fused_asm.py and test_gpu_k4_stream.py, written from the selection code as it was
 * spread over the engine and confirmed on the GPU against that engine (profiles/ll_plan_refactor_ab.json); the rows without
 * the stream stand for a failed allocation of it, which no option asks for: those are from the code alone */
static std::string check_k4_table()
{
    enum { CAT8, BAL32, BAL64, IRREG };
    struct Row { int tree, nchar, C; long S, mode, fasm, spl; bool allow; PlkK4Variant variant; int tile; };
    const Row rows[] = {
        {CAT8, 5, 4, 300, 1, 1, 0, true, PLK_K4_V4S, 1536},        /* the default: streamed codes */
        {CAT8, 5, 4, 300, 7, 1, 0, true, PLK_K4_V4S, 1536},
        {CAT8, 5, 4, 300, 1, 1, 0, false, PLK_K4_V4, 1024},        /* no stream: one round of either tile, the smaller first */
        {CAT8, 5, 4, 10000000, 1, 1, 0, false, PLK_K4_V4, 1536},   /* 26 rounds of 1536 (x 1.3 = 33.8) against 39 of 1024 */
        {CAT8, 5, 4, 1250000, 1, 1, 0, false, PLK_K4_V4, 1024},    /* 4 rounds of 1536 (5.2) against 5 of 1024 */
        {CAT8, 5, 4, 300, 6, 1, 0, true, PLK_K4_V4, 1536},
        {CAT8, 5, 4, 300, 5, 1, 0, true, PLK_K4_V4, 1024},
        {CAT8, 5, 4, 300, 2, 1, 0, true, PLK_K4_ASM_PT, 1024},
        {CAT8, 5, 4, 300, 3, 1, 0, true, PLK_K4_ASM_PT, 512},
        {CAT8, 5, 4, 300, 0, 1, 0, true, PLK_K4_ASM, 256},
        {CAT8, 5, 4, 300, 0, 0, 0, true, PLK_K4_CPP, 256},
        {CAT8, 5, 4, 300, 1, 0, 0, true, PLK_K4_CPP, 256},         /* pair tables need the assembly option */
        {CAT8, 5, 4, 300, 1, 1, 2, true, PLK_K4_CPP, 512},         /* two sites per lane: the C++ interpreter only */
        {CAT8, 16, 4, 129, 7, 1, 0, true, PLK_K4_V4S, 1536},
        {CAT8, 4, 1, 129, 7, 1, 0, true, PLK_K4_V4S, 1536},
        {BAL32, 16, 2, 129, 7, 1, 0, true, PLK_K4_V4, 1024},       /* 128 KB of tables per category: two do not fit, a tile kernel */
        {BAL32, 16, 2, 129, 6, 1, 0, true, PLK_K4_V4, 1536},
        {BAL32, 5, 1, 300, 1, 1, 0, true, PLK_K4_V4S, 1536},
        {BAL32, 5, 1, 300, 0, 1, 0, true, PLK_K4_ASM, 256},
        {BAL64, 5, 4, 300, 1, 1, 0, true, PLK_K4_ASM, 256},        /* 5 stack slots: no pair tables */
        {BAL64, 5, 4, 300, 1, 0, 0, true, PLK_K4_CPP, 256},
        {BAL64, 5, 4, 300, 1, 1, 2, true, PLK_K4_CPP, 512},
        {IRREG, 7, 4, 300, 1, 1, 0, true, PLK_K4_V4S, 1536},
        {IRREG, 7, 4, 300, 6, 1, 0, true, PLK_K4_V4, 1536},
        {IRREG, 17, 2, 300, 1, 1, 0, true, PLK_K4_ASM, 256},       /* 17 definitions: no pair tables, 8-bit staged codes */
        {IRREG, 17, 2, 300, 1, 0, 0, true, PLK_K4_CPP, 256},
    };
    Tree trees[4];
    std::vector<char> has[4];
    caterpillar_tree(8, trees[CAT8]); balanced_tree(32, trees[BAL32]); balanced_tree(64, trees[BAL64]);
    irregular_tree(trees[IRREG], has[IRREG]);
    for (int q = 0; q < 3; q++) has[q].assign(trees[q].N, 0);
    int r = 0;
    for (const Row &w : rows) {
        const Tree &t = trees[w.tree];
        PlkProgram pg;
        plk_program_build(t.N, t.ip.data(), t.ix.data(), t.pre.data(), has[w.tree].data(), pg);
        K4Formats F;
        const PlkK4Choice ch = k4_choose(t, pg, w.nchar, w.C, w.S, w.mode, w.fasm, w.spl, w.allow, F);
        if (ch.variant != w.variant || ch.tile != w.tile || !ch.bad.empty())
            return plk_fmt("k4 table row %ld: variant %ld at tile %ld", r, ch.variant, ch.tile) + plk_fmt(", expected variant %ld at tile %ld ", w.variant, w.tile) + ch.bad;
        r++;
    }
    return "";
}

/* the sweep over the seeded random trees' subset is run from main; here the constructed trees and the outcome counts */
static std::string check_k4_constructed()
{
    const int nchars[4] = {4, 5, 16, 17};
    std::string bad;
    Tree t;
    /* 90 leaves with 16 definitions: 1024-site tiles fit, 512- and 1536-site tiles do not (forced modes 3 and 6 fall through) */
    const int cats[6] = {2, 8, 40, 90, 300, 2000}, bals[4] = {8, 32, 64, 256};
    for (int n : cats) { caterpillar_tree(n, t); bad = check_k4_choice(t, std::vector<char>(t.N, 0), nchars, 4); if (!bad.empty()) return plk_fmt("caterpillar %ld: ", n) + bad; }
    for (int n : bals) { balanced_tree(n, t); bad = check_k4_choice(t, std::vector<char>(t.N, 0), nchars, 4); if (!bad.empty()) return plk_fmt("balanced %ld: ", n) + bad; }
    /* k_ll_fused4<16, 1> needs more than 8 stack slots and an LDS image that still fits: the tree of the GPU tests' "deep"
     * workload (tests/helpers.py, deep_workload: the full binary tree over 512 unary nodes with one leaf each, stack need 9)
     * with its ONE character definition, outside the nchar values of the sweep */
    const int one[1] = {1};
    std::vector<int> parent(1535, 0);
    for (int i = 1; i < 1023; i++) parent[i] = (i - 1) / 2;
    for (int i = 0; i < 512; i++) parent[1023 + i] = 511 + i;
    tree_from_parents(parent, t);
    bad = check_k4_choice(t, std::vector<char>(t.N, 0), one, 1);
    if (!bad.empty()) return "deep tree, one definition: " + bad;
    return "";
}

/* The rescaling bound on constructed wide nodes, each through every check of check_tree, and the negative control: on the
 * m-leaf star the end-of-node rule lets the root vector take all m factors, and the replay says so. */
static std::string check_scale_constructed()
{
    Tree t;
    std::string bad;
    auto run_case = [&](const std::vector<int> &parent, const char *what, int wide, bool data_on_wide) -> std::string {
        if (!tree_from_parents(parent, t)) return std::string(what) + ": not a tree";
        std::vector<char> has(t.N, 0);
        if (data_on_wide) has[wide] = 1;
        PlkProgram pg;
        plk_program_build(t.N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
        if (!pg.mid_scale_node[wide] || pg.mid_scales < 1) return std::string(what) + ": the wide node is not rescaled inside";
        const std::string b = check_tree(t, has, 5);
        return b.empty() ? b : std::string(what) + ": " + b;
    };
    /* a star of 1000 leaves */
    if (!(bad = run_case(std::vector<int>(1001, 0), "star of 1000", 0, false)).empty()) return bad;
    /* a root with 40 leaf children and 40 internal children (cherries) */
    {
        std::vector<int> parent(1 + 40 + 40 + 80, 0);
        for (int i = 0; i < 80; i++) parent[81 + i] = 41 + i / 2;
        if (!(bad = run_case(parent, "40 leaves and 40 cherries under one node", 0, true)).empty()) return bad;
    }
    /* a caterpillar of 8 leaves whose node at depth 3 (node 6) also has 60 leaf children and 6 cherries, and below them a
     * unary node */
    {
        std::vector<int> parent(15, 0);
        for (int i = 1; i < 15; i++) parent[i] = i % 2 ? i - 1 : i - 2;
        for (int i = 0; i < 60; i++) parent.push_back(6);
        const int c0 = (int)parent.size();
        for (int i = 0; i < 6; i++) parent.push_back(6);
        for (int i = 0; i < 12; i++) parent.push_back(c0 + i / 2);
        const int un = (int)parent.size();
        parent.push_back(6);       /* unary node ... */
        parent.push_back(un);      /* ... over one leaf */
        if (!(bad = run_case(parent, "wide node at depth 3 of a caterpillar", 6, true)).empty()) return bad;
    }
    /* the benign shapes of tests/test_gpu_polytomy.py are rescaled inside too: a 40-leaf star, and a root over three 8-leaf
     * caterpillars (every other node binary; runs of 16 + 16 + 16) */
    if (!(bad = run_case(std::vector<int>(41, 0), "star of 40", 0, false)).empty()) return bad;
    {
        std::vector<int> parent(1, 0);
        for (int c = 0; c < 3; c++) {
            const int top = (int)parent.size();
            parent.push_back(0);
            for (int i = 1; i < 15; i++) parent.push_back(top + (i % 2 ? i - 1 : i - 2));
        }
        if (!(bad = run_case(parent, "root over three 8-leaf caterpillars", 0, false)).empty()) return bad;
    }
    /* stars around the bound: none inside up to PLK_SCALE_RUN leaves, one per PLK_SCALE_RUN leaves beyond */
    const int ms[] = {2, 16, PLK_SCALE_RUN, PLK_SCALE_RUN + 1, 2 * PLK_SCALE_RUN, 2 * PLK_SCALE_RUN + 1, 70, 300, 1000};
    for (int m : ms) {
        tree_from_parents(std::vector<int>(m + 1, 0), t);
        const std::vector<char> has(t.N, 0);
        PlkProgram pg, old;
        plk_program_build(t.N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
        program_build_end_of_node_rule(t, has, old);
        int nscale = 0;
        for (const plk_op2 &o : pg.ops) nscale += (o.x & 0xff) == OP_SCALE;
        const int inside = (m - 1) / PLK_SCALE_RUN, want = inside + (inside > 0 || m >= 16 ? 1 : 0);
        if (nscale != want) return plk_fmt("star of %ld: %ld OP_SCALE, expected %ld", m, nscale, want);
        if (max_unscaled_run(pg) != std::min(m, PLK_SCALE_RUN)) return plk_fmt("star of %ld: run of %ld", m, max_unscaled_run(pg));
        /* negative control */
        if (max_unscaled_run(old) != m) return plk_fmt("negative control: the replay reports %ld on the end-of-node program of the %ld-leaf star", max_unscaled_run(old), m);
    }
    return "";
}

int main(int argc, char **argv)
{
    long ntrees = 0;
    { const std::string bad = check_chunk_planner(); if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; } }
    { const std::string bad = check_k4_table(); if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; } }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
        int N, nchar;
        while (fscanf(f, "%d %d", &N, &nchar) == 2) {
            if (N < 2) return 2;
            std::vector<int> ea(N - 1), eb(N - 1);
            for (int e = 0; e < N - 1; e++) if (fscanf(f, "%d %d", &ea[e], &eb[e]) != 2) return 2;
            char bar[4];
            if (fscanf(f, "%3s", bar) != 1 || bar[0] != '|') return 2;
            std::vector<char> has(N);
            for (int a = 0; a < N; a++) { int v; if (fscanf(f, "%d", &v) != 1) return 2; has[a] = (char)v; }
            Tree t;
            if (!make_tree(N, ea, eb, t)) { fprintf(stderr, "tree %ld is not a rooted tree\n", ntrees); return 1; }
            for (int a = 0; a < N; a++) if (t.ip[a + 1] == t.ip[a]) has[a] = 0;   /* leaves are tips, not NODE_MUL */
            const std::string bad = check_tree(t, has, nchar);
            if (!bad.empty()) { fprintf(stderr, "tree %ld (N = %d, nchar = %d): %s\n", ntrees, N, nchar, bad.c_str()); return 1; }
            ntrees++;
        }
        fclose(f);
        printf("ok %ld %ld\n", ntrees, g_ops);
        return 0;
    }
    std::mt19937_64 rng(20250355);
    auto rnd = [&](int n) { return (int)(rng() % (unsigned long long)n); };
    const int nchars[] = {1, 2, 5, 16, 17, 64, 255, 256};
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
            case 0: parent = rnd(i); break;                                   /* random recursive tree (multifurcating) */
            case 1: parent = i - 1; break;                                    /* chain: every node has one child */
            case 2: parent = (i - 1) / 2; break;                              /* complete binary */
            case 3: parent = i % 2 ? i - 1 - (i > 1) : i - 2; if (parent < 0) parent = 0; break;   /* caterpillar */
            case 4: parent = 0; break;                                        /* star */
            case 5: parent = rnd(10) < 7 ? rnd(i) : std::max(0, i - 1 - rnd(std::min(i, 3))); break;  /* the differential generator's mix */
            case 6: parent = (i - 1) / 3; break;                              /* ternary */
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
        std::string bad = check_tree(t, has, nchars[rnd(8)]);
        if (bad.empty() && iter % 40 == 3) { const int k4_nchars[4] = {4, 5, 16, 17}; bad = check_k4_choice(t, has, k4_nchars, 4); }
        if (!bad.empty()) { fprintf(stderr, "iteration %d (shape %d, N = %d): %s\n", iter, shape, N, bad.c_str()); return 1; }
        ntrees++;
    }
    /* deep stacks: complete binary trees up to 4096 leaves (stack depth beyond every register variant) */
    for (int d = 2; d <= 12; d++) {
        const int N = (1 << (d + 1)) - 1;
        std::vector<int> ea(N - 1), eb(N - 1);
        for (int i = 1; i < N; i++) { ea[i - 1] = (i - 1) / 2; eb[i - 1] = i; }
        Tree t;
        make_tree(N, ea, eb, t);
        std::vector<char> has(N, 0);
        const std::string bad = check_tree(t, has, 5);
        if (!bad.empty()) { fprintf(stderr, "balanced depth %d: %s\n", d, bad.c_str()); return 1; }
        ntrees++;
    }
    { const std::string bad = check_scale_constructed(); if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; } }
    fprintf(stderr, "rescaling: %ld trees with an OP_SCALE inside a node, %ld with the end-of-node rule's program\n", g_mid_scaled, g_same_as_before);
    if (g_mid_scaled < 20 || g_same_as_before < 3000) { fprintf(stderr, "rescaling: the sweep does not reach both kinds of tree\n"); return 1; }
    /* the k = 4 choice on constructed trees, then: every outcome of the choice was reached (the sweep cannot pass vacuously) */
    { const std::string bad = check_k4_constructed(); if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; } }
    for (int q = 0; q < OUT_COUNT; q++) {
        fprintf(stderr, "k4 choice: %-16s %ld\n", OUT_NAME[q], g_outcome[q]);
        if (!g_outcome[q]) { fprintf(stderr, "k4 choice: outcome \"%s\" was never chosen\n", OUT_NAME[q]); return 1; }
    }
    /* ... and so was a forced mode whose tile does not fit while another would.  Modes 3 (512-site tiles) and 6 (1536) have
     * such cases.  Modes 2 and 5 (1024 sites) cannot: the image of a 1536-site tile is larger under the same limit, twice the
     * image of a 512-site tile under half the limit is no smaller than that of a 1024-site tile, and the other 1024-site kernel
     * has the same image -- should a case turn up after all, it has to be required here too. */
    for (int mode : {2, 3, 5, 6}) {
        fprintf(stderr, "k4 choice: forced mode %d fell through past a fitting tile kernel %ld times\n", mode, g_forced_fell_through[mode]);
        if ((g_forced_fell_through[mode] == 0) == (mode == 3 || mode == 6)) { fprintf(stderr, "k4 choice: forced mode %d: fall-through count\n", mode); return 1; }
    }
    printf("ok %ld %ld\n", ntrees, g_ops);
    return 0;
}
