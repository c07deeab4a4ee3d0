/*
 * tests/synccheck_main.cpp -- CPU driver for the barrier default of the streamed k = 4 kernel (plk_v4s_auto_sync and the
 * sync / sync_auto fields of plk_k4_stream in phyly_amd/csrc/plk_program.h: the value that is launched), built with
 * AddressSanitizer + UBSan by tests/test_k4_sync_host.py.
 *
 * Argument: the tree of BASELINE config 3 as tests/pairmulcheck_main.cpp reads it (nchar 5; every leaf is given the four
 * codes of fully observed data, so that four-leaf tables qualify).  For a list of (categories, sites, CUs) it asks
 * plk_k4_choose for the plan and plk_k4_stream, every capability given, for the formats that run, and requires:
 *   - without sync bits: sync_auto, and sync = 0 exactly where one category is resident at a time (one rate category, or a
 *     plan with a group per category) and the matrix stream left by the plan's tables plus the op words fit 16 KB, else 2;
 *   - both outcomes occur in the list, and BASELINE config 3 itself (4 categories, 10M sites, 256 CUs) is a plan of four
 *     groups without the barrier, and so is the same alignment cut for 8 GPUs (1.25M sites, 4 units a wave);
 *   - + 16, + 32, + 16 + 32 (+ 32 wins, as it always did) and + 65536 give 1, 0, 0 and 2 whatever the plan, and sync_auto is off;
 *   - the rule's edges: a second resident category, one byte more than 16 KB.
 * Prints "ok <plans without the barrier> <plans with it>" and exits 0, or the first failure and exits 1.
 */
#include <cstdio>
#include <string>
#include <vector>

#include "plk_program.h"

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: synccheck TREE\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int N = 0;
    bool ok = fscanf(f, "%d", &N) == 1 && N >= 2 && N < 100000;
    std::vector<int> ip, ix, pre;
    if (ok) {
        ip.resize(N + 1); ix.resize(N - 1); pre.resize(N);
        for (int &v : ip) ok = ok && fscanf(f, "%d", &v) == 1;
        for (int &v : ix) ok = ok && fscanf(f, "%d", &v) == 1 && v >= 0 && v < N;
        for (int &v : pre) ok = ok && fscanf(f, "%d", &v) == 1 && v >= 0 && v < N;
        ok = ok && ip[0] == 0 && ip[N] == N - 1;
        for (int a = 0; ok && a < N; a++) ok = ip[a + 1] >= ip[a];
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: not a tree file\n", argv[1]); return 2; }
    const int nchar = 5;
    std::vector<char> has(N, 0);
    std::vector<int> masks(N, 0);
    for (int a = 0; a < N; a++) if (ip[a + 1] == ip[a]) masks[a] = 0xf;
    PlkProgram pg;
    plk_program_build(N, ip.data(), ix.data(), pre.data(), has.data(), pg);

    if (plk_v4s_auto_sync(1, 127, 0) != 0 || plk_v4s_auto_sync(1, 127, 1) != 2 || plk_v4s_auto_sync(2, 1, 16) != 2 || plk_v4s_auto_sync(1, 35, 512) != 0 || plk_v4s_auto_sync(4, 35, 512) != 2) {
        fprintf(stderr, "plk_v4s_auto_sync: the rule's edges\n"); return 1;
    }
    /* expect: written down from the plans, not from the rule -- at 10M and 2.5M sites one resident image holds every table and the
     * plan is a group per category (2, 3 or 4 of them); one rate category is one resident category with or without tables;
     * 1.25M sites, and 4685 on one CU, are 4 units a wave, where a phase costs little and the plan is the same; 1000 sites are
     * below the gate (no tables, every category resident) */
    struct Case { int C; long S; int cus; int expect; };
    const Case cases[] = {{4, 10000000, 256, 0}, {4, 1250000, 256, 0}, {4, 2500000, 256, 0}, {1, 10000000, 256, 0}, {1, 1000, 256, 0}, {4, 1000, 256, 2}, {2, 1000, 256, 2}, {3, 1000, 256, 2}, {4, 4685, 1, 0},
                          {2, 10000000, 256, 0}, {3, 10000000, 256, 0}};
    long n0 = 0, n2 = 0;
    for (const Case &cs : cases) {
        PlkK4Shape sh = {nchar, cs.C, cs.S, cs.cus, 1, 1, 0, {0, 0, 0}};
        sh.node_codes = masks.data();
        PlkFused fu; PlkFusedPT fpt; PlkFusedV4 fv4; PlkFusedV4S fv4s;
        const PlkK4Choice chosen = plk_k4_choose(N, ip.data(), ix.data(), pg, sh, true, fu, fpt, fv4, fv4s);
        if (!chosen.bad.empty() || chosen.variant != PLK_K4_V4S) { fprintf(stderr, "C %d S %ld: not the streamed form (%s)\n", cs.C, cs.S, chosen.bad.c_str()); return 1; }
        const size_t checked_nmat = fpt.mat_edge.size();
        const PlkK4Stream ch = plk_k4_stream(N, ip.data(), ix.data(), pg, sh, chosen, PlkK4StreamCaps(), fpt, fv4s);
        if (!ch.note.empty()) { fprintf(stderr, "C %d S %ld: %s\n", cs.C, cs.S, ch.note.c_str()); return 1; }
        const bool tables = ch.triple.nodes + ch.triple.quads > 0;
        const int Cg = tables && ch.triple.Cg > 0 ? ch.triple.Cg : cs.C;
        /* the matrix stream the plan's tables leave: counted from the plan, and what the format that runs must hold */
        size_t nmat = checked_nmat;
        if (tables) { nmat -= (size_t)ch.triple.nodes; for (int s : ch.triple.quad_shape) nmat -= s == PLK_V4Q_A ? 2 : 1; }
        if (nmat != fpt.mat_edge.size()) { fprintf(stderr, "C %d S %ld: %zu matrices run, the plan leaves %zu\n", cs.C, cs.S, fpt.mat_edge.size(), nmat); return 1; }
        const int want = Cg == 1 && (nmat + 1) * 128 + ch.stride() * 4 <= 16384 ? 0 : 2;
        if (!ch.sync_auto || ch.sync != want) { fprintf(stderr, "C %d S %ld CUs %d: sync %d (auto %d), %d expected with %d resident categories\n", cs.C, cs.S, cs.cus, ch.sync, (int)ch.sync_auto, want, Cg); return 1; }
        if (ch.sync != cs.expect) { fprintf(stderr, "C %d S %ld CUs %d: sync %d, the plan (%d groups) was expected to give %d\n", cs.C, cs.S, cs.cus, ch.sync, ch.triple.groups, cs.expect); return 1; }
        (ch.sync ? n2 : n0)++;
        if (cs.C == 4 && cs.S == 10000000 && (ch.triple.groups != 4 || ch.sync != 0)) { fprintf(stderr, "config 3: %d groups, sync %d\n", ch.triple.groups, ch.sync); return 1; }
        if (cs.C == 4 && cs.S == 1250000 && (ch.triple.groups != 4 || ch.sync != 0)) { fprintf(stderr, "config 3 at 1.25M sites: %d groups, sync %d\n", ch.triple.groups, ch.sync); return 1; }
        if (cs.C == 1 && ch.sync != 0) { fprintf(stderr, "one rate category with the barrier\n"); return 1; }
        const long bits[4] = {16, 32, 48, 65536};
        const int forced[4] = {1, 0, 0, 2};
        for (int b = 0; b < 4; b++) {
            sh.pair_tables = 1 + bits[b];
            const PlkK4Choice forced_choice = plk_k4_choose(N, ip.data(), ix.data(), pg, sh, true, fu, fpt, fv4, fv4s);
            const PlkK4Stream cf = plk_k4_stream(N, ip.data(), ix.data(), pg, sh, forced_choice, PlkK4StreamCaps(), fpt, fv4s);
            if (forced_choice.sync_auto || forced_choice.sync != forced[b] || cf.sync_auto || cf.sync != forced[b]) { fprintf(stderr, "C %d S %ld: + %ld gives sync %d\n", cs.C, cs.S, bits[b], cf.sync); return 1; }
        }
    }
    if (!n0 || !n2) { fprintf(stderr, "only one outcome in the list\n"); return 1; }
    printf("ok %ld %ld\n", n0, n2);
    return 0;
}
