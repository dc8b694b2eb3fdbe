// post_host.cpp -- SURVEY.md 8f row N2, second half: the reference's bridge-based heuristics for ONE frame, on the host.
//
// The shipped inference configuration (config/config_inference.yaml:6-8) runs, after the threshold, PRUNING -> ROUNDING -> PRUNING ->
// SPLITTING (inference.py:306-345).  The device chain (csrc/postprocess.cuh) covers threshold, pruning, flow counts and clusters and raises
// two trigger bits per frame -- a node with flow > 3 (libs/utils.py:58-59), a cluster with more than four members (libs/utils.py:321);
// only frames that raise one need what is below, and SURVEY.md 8f leaves that on the CPU: graphs of <= 34 nodes, bridge searches, loops
// whose trip count depends on the data.  `gnncca_post_finalize_frame_host` is utils.compute_rounding (libs/utils.py:25-173),
// utils.remove_edges_single_direction (387-404), utils.disjoint_big_clusters (319-386) and utils.compute_SCC_and_Clusters (295-317) in
// that order, with the reference's OBSERVABLE behaviour -- its artefacts included, because they decide which edges go:
//   * cluster labels are positions in [strongly connected components in networkx's generation order, stably sorted by size] + [untouched
//     nodes in id order]; the splitting step works on the FIRST label with more than four members and re-reads "label l" in every
//     re-labelling -- so scc_generation_order() below follows networkx's algorithm (Nuutila's variant of Tarjan, nodes and successors in
//     insertion order), not just any SCC routine;
//   * rounding looks for bridges in the graph it was called with, every round (the reference never refreshes `predicted_active_edges`);
//   * splitting removes EVERY edge whose probability equals the minimum it found, looks for bridges in the whole frame and not in the big
//     cluster, and drops its recursive call's result except for that call's first in-place removal.
// Written from the reference's behaviour, checked against tests/golden/post2_heuristics.npz (the reference's own functions) and against
// oracle/post_oracle.py.
//
// Round 6: the synthetic model of bench.py flags 58 of 64 frames per batch, and this file was 1.0 ms of a 1.1 ms batch.
// (i) No allocation per frame: every table lives in a thread-local `Solver` whose vectors keep their capacity; adjacency is CSR built by
// counting, pair sets are stamped dense maps (n <= 2048; hash sets beyond), stable sorts of <= 64 sets are insertion sorts.  The first
// version built vector<vector<int>> adjacency and unordered_sets per call: 77-115 us per Terrace frame and NO scaling over threads (the
// allocator on the first box measured), now 28-30 us on one thread of the same host and 6.4x faster on eight.  (ii) The recursive call of the splitting step is evaluated only as far as the reference KEEPS it:
// its first in-place removal (everything after it works on a new object whose value is dropped, libs/utils.py:382-384).  (iii) A
// persistent pool of host threads with an asynchronous batch interface (gnncca_post_pool_*): a batch's trigger words, edges, probabilities
// and pruned predictions arrive in pinned memory behind a HIP event; a pool thread waits for the event, lists the flagged frames and the
// pool finalizes them while the caller enqueues the next batch's GPU chain.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "internal.h"

namespace {

typedef std::vector<int64_t> Pred;

// ordered node pairs (u, v) -> int value: a stamped dense n x n table for frames (n <= 2048: 16 MB at most, kept by the thread), a hash map
// beyond.  reset() costs nothing (the stamp advances); absent = -1.
struct PairTable {
    int n = 0;
    bool dense = true;
    uint32_t cur = 0;
    std::vector<uint32_t> stamp;
    std::vector<int> val;
    std::unordered_map<uint64_t, int> sparse;
    void reset(int n_) {
        n = n_;
        dense = n <= 2048;
        if (!dense) {
            sparse.clear();
            return;
        }
        const size_t need = (size_t)n * n;
        if (stamp.size() < need) stamp.assign(need, 0), val.assign(need, 0), cur = 0;
        if (++cur == 0) std::fill(stamp.begin(), stamp.end(), 0u), cur = 1;
    }
    bool insert(int u, int v, int value = 1) {   // true if new (an existing entry keeps its value)
        if (dense) {
            const size_t i = (size_t)u * n + v;
            if (stamp[i] == cur) return false;
            stamp[i] = cur, val[i] = value;
            return true;
        }
        return sparse.emplace((uint64_t)u * (uint64_t)n + (uint64_t)v, value).second;
    }
    int get(int u, int v) const {
        if (dense) {
            const size_t i = (size_t)u * n + v;
            return stamp[i] == cur ? val[i] : -1;
        }
        auto q = sparse.find((uint64_t)u * (uint64_t)n + (uint64_t)v);
        return q == sparse.end() ? -1 : q->second;
    }
    bool has(int u, int v) const { return get(u, v) >= 0; }
};

// One frame's tables + every scratch buffer of the heuristics; thread-local, reused from frame to frame (nothing below allocates once
// the vectors have grown to the largest frame the thread has seen).
struct Solver {
    int n = 0, E = 0;
    const float* probs = nullptr;
    std::vector<int> eu, ev;                                   // frame-local endpoints
    std::vector<int> out_ptr, out_idx, in_ptr, in_idx;         // edge ids by source / by target node, ascending
    PairTable pairs, bridge_tab, first_tab;
    std::vector<int> bridge_list;                              // (u, v) of both orientations of every bridge of the last bridge_set()
    // digraph (networkx.DiGraph(edge list): nodes in order of first appearance, successors in insertion order, parallel edges once)
    std::vector<int> g_nodes, g_ptr, g_succ, g_cur;
    std::vector<char> g_present, keep;
    // SCC
    std::vector<int> preorder, lowlink, it, sccq, queue, scc_ptr, scc_nodes, order;
    std::vector<char> found;
    // bridges
    std::vector<int> u_ptr, u_adj, u_cur, disc, low, parent, stack;
    // rounding / splitting
    std::vector<int> fo, fi, act, remove, ids, count;
    std::vector<char> on_bridge;
    Pred work;

    bool load(const int64_t* src, const int64_t* dst, int64_t base, int64_t n_nodes, int64_t n_edges, const float* p) {
        n = (int)n_nodes, E = (int)n_edges, probs = p;
        eu.resize(E), ev.resize(E);
        out_ptr.assign(n + 1, 0), in_ptr.assign(n + 1, 0);
        for (int k = 0; k < E; ++k) {
            const int64_t u = src[k] - base, v = dst[k] - base;
            if (u < 0 || u >= n_nodes || v < 0 || v >= n_nodes) return false;
            eu[k] = (int)u, ev[k] = (int)v;
            out_ptr[u + 1]++, in_ptr[v + 1]++;
        }
        for (int v = 0; v < n; ++v) out_ptr[v + 1] += out_ptr[v], in_ptr[v + 1] += in_ptr[v];
        out_idx.resize(E), in_idx.resize(E);
        g_cur.assign(out_ptr.begin(), out_ptr.end() - 1), u_cur.assign(in_ptr.begin(), in_ptr.end() - 1);
        for (int k = 0; k < E; ++k) out_idx[g_cur[eu[k]]++] = k, in_idx[u_cur[ev[k]]++] = k;
        return true;
    }

    void digraph(const std::vector<int>& a) {
        g_nodes.clear();
        g_present.assign(n, 0);
        g_ptr.assign(n + 1, 0);
        keep.resize(a.size());
        pairs.reset(n);
        for (size_t i = 0; i < a.size(); ++i) {
            const int u = eu[a[i]], v = ev[a[i]];
            if (!g_present[u]) g_present[u] = 1, g_nodes.push_back(u);
            if (!g_present[v]) g_present[v] = 1, g_nodes.push_back(v);
            keep[i] = (char)pairs.insert(u, v);
            if (keep[i]) g_ptr[u + 1]++;
        }
        for (int v = 0; v < n; ++v) g_ptr[v + 1] += g_ptr[v];
        g_succ.resize(g_ptr[n]);
        g_cur.assign(g_ptr.begin(), g_ptr.end() - 1);
        for (size_t i = 0; i < a.size(); ++i)
            if (keep[i]) g_succ[g_cur[eu[a[i]]]++] = ev[a[i]];
    }

    // networkx.strongly_connected_components in generation order (networkx/algorithms/components/strongly_connected.py) -> scc_ptr / scc_nodes
    void scc_generation_order() {
        preorder.assign(n, 0), lowlink.assign(n, 0), found.assign(n, 0);
        it.assign(g_ptr.begin(), g_ptr.end() - 1);            // the node's neighbour iterator keeps its position across visits
        sccq.clear(), scc_ptr.assign(1, 0), scc_nodes.clear();
        int i = 0;
        for (int source : g_nodes) {
            if (found[source]) continue;
            queue.assign(1, source);
            while (!queue.empty()) {
                const int v = queue.back();
                if (!preorder[v]) preorder[v] = ++i;
                bool done = true;
                while (it[v] < g_ptr[v + 1]) {
                    const int w = g_succ[it[v]++];
                    if (!preorder[w]) {
                        queue.push_back(w);
                        done = false;
                        break;
                    }
                }
                if (!done) continue;
                lowlink[v] = preorder[v];
                for (int q = g_ptr[v]; q < g_ptr[v + 1]; ++q) {
                    const int w = g_succ[q];
                    if (!found[w]) lowlink[v] = std::min(lowlink[v], preorder[w] > preorder[v] ? lowlink[w] : preorder[w]);
                }
                queue.pop_back();
                if (lowlink[v] == preorder[v]) {
                    scc_nodes.push_back(v), found[v] = 1;
                    while (!sccq.empty() && preorder[sccq.back()] > preorder[v]) found[sccq.back()] = 1, scc_nodes.push_back(sccq.back()), sccq.pop_back();
                    scc_ptr.push_back((int)scc_nodes.size());
                } else {
                    sccq.push_back(v);
                }
            }
        }
    }

    // utils.compute_SCC_and_Clusters: out[v] = position of v's set in [SCCs stably sorted by size] + [untouched nodes in id order]
    int cluster_ids(const std::vector<int>& a, std::vector<int>& out) {
        digraph(a);
        scc_generation_order();
        const int S = (int)scc_ptr.size() - 1;
        order.resize(S);
        for (int s = 0; s < S; ++s) order[s] = s;
        auto size_of = [&](int s) { return scc_ptr[s + 1] - scc_ptr[s]; };
        if (S <= 64) {                                          // stable insertion sort: no temporary buffer
            for (int s = 1; s < S; ++s) {
                const int x = order[s], sx = size_of(x);
                int q = s - 1;
                while (q >= 0 && size_of(order[q]) > sx) order[q + 1] = order[q], --q;
                order[q + 1] = x;
            }
        } else {
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return size_of(x) < size_of(y); });
        }
        out.assign(n, 0);
        int c = 0;
        for (int s : order) {
            for (int q = scc_ptr[s]; q < scc_ptr[s + 1]; ++q) out[scc_nodes[q]] = c;
            ++c;
        }
        for (int v = 0; v < n; ++v)
            if (!g_present[v]) out[v] = c++;
        return c;
    }

    // both orientations of every bridge of the undirected graph of the active edges -> bridge_tab / bridge_list (which bridges exist does
    // not depend on the order the search visits neighbours in)
    void bridge_set(const std::vector<int>& a) {
        u_ptr.assign(n + 1, 0);
        keep.resize(a.size());
        pairs.reset(n);
        for (size_t i = 0; i < a.size(); ++i) {
            const int u = eu[a[i]], v = ev[a[i]];
            keep[i] = (char)(u != v && pairs.insert(std::min(u, v), std::max(u, v)));
            if (keep[i]) u_ptr[u + 1]++, u_ptr[v + 1]++;
        }
        for (int v = 0; v < n; ++v) u_ptr[v + 1] += u_ptr[v];
        u_adj.resize(u_ptr[n]);
        u_cur.assign(u_ptr.begin(), u_ptr.end() - 1);
        for (size_t i = 0; i < a.size(); ++i)
            if (keep[i]) {
                const int u = eu[a[i]], v = ev[a[i]];
                u_adj[u_cur[u]++] = v, u_adj[u_cur[v]++] = u;
            }
        bridge_tab.reset(n);
        bridge_list.clear();
        disc.assign(n, 0), low.assign(n, 0), parent.assign(n, -1);
        u_cur.assign(u_ptr.begin(), u_ptr.end() - 1);
        int t = 0;
        for (int root = 0; root < n; ++root) {
            if (disc[root] || u_ptr[root] == u_ptr[root + 1]) continue;
            disc[root] = low[root] = ++t;
            stack.assign(1, root);
            while (!stack.empty()) {
                const int v = stack.back();
                if (u_cur[v] < u_ptr[v + 1]) {
                    const int w = u_adj[u_cur[v]++];
                    if (w == parent[v]) continue;              // (simple graph: the one edge back to the parent)
                    if (disc[w]) {
                        low[v] = std::min(low[v], disc[w]);
                    } else {
                        parent[w] = v;
                        disc[w] = low[w] = ++t;
                        stack.push_back(w);
                    }
                } else {
                    stack.pop_back();
                    const int p = parent[v];
                    if (p >= 0) {
                        low[p] = std::min(low[p], low[v]);
                        if (low[v] > disc[p]) {
                            bridge_tab.insert(p, v), bridge_tab.insert(v, p);
                            bridge_list.push_back(p), bridge_list.push_back(v), bridge_list.push_back(v), bridge_list.push_back(p);
                        }
                    }
                }
            }
        }
    }

    // Every routine below works on the LIST of active edges (`a`, ascending edge ids: the order the reference's np.nonzero / list
    // comprehensions produce) next to the 0 / 1 vector `p`; an edge that goes is zeroed in `p` and the list is compacted -- a frame has 343
    // edges and ~70 active ones, and the heuristics' loops run tens of rounds (the first version re-scanned all E edges eight times a round).
    void compact(const Pred& p, std::vector<int>& a) const {
        size_t w = 0;
        for (size_t i = 0; i < a.size(); ++i)
            if (p[a[i]] == 1) a[w++] = a[i];
        a.resize(w);
    }

    // utils.remove_edges_single_direction, in place: an active edge survives iff its reverse is active too
    void prune(Pred& p, std::vector<int>& a) {
        pairs.reset(n);
        for (int k : a) pairs.insert(eu[k], ev[k]);
        bool any = false;
        for (int k : a)
            if (!pairs.has(ev[k], eu[k])) p[k] = 0, any = true;
        if (any) compact(p, a);
    }

    void flows(const std::vector<int>& a) {
        fo.assign(n, 0), fi.assign(n, 0);
        for (int k : a) fo[eu[k]]++, fi[ev[k]]++;
    }
    bool violated() const {
        for (int v = 0; v < n; ++v)
            if (fo[v] > 3 || fi[v] > 3) return true;
        return false;
    }

    // utils.compute_rounding on (p, a) in place; false where the reference returns [] (no node with flow > 3: the caller keeps its predictions)
    bool rounding(Pred& p, std::vector<int>& a) {
        flows(a);
        if (!violated()) return false;
        bridge_set(a);                                          // of the graph the call came with, every round
        const bool have_bridges = !bridge_list.empty();
        if (have_bridges) {
            on_bridge.assign(E, 0);
            for (int k : a) on_bridge[k] = (char)bridge_tab.has(eu[k], ev[k]);
        }
        for (;;) {
            remove.clear();
            if (have_bridges) {
                for (int side = 0; side < 2; ++side)
                    for (int v = 0; v < n; ++v) {
                        if ((side == 0 ? fo[v] : fi[v]) <= 3) continue;
                        const std::vector<int>& ptr = side == 0 ? out_ptr : in_ptr;
                        const std::vector<int>& idx = side == 0 ? out_idx : in_idx;
                        for (int q = ptr[v]; q < ptr[v + 1]; ++q)   // ascending edge ids, as np.intersect1d returns them
                            if (p[idx[q]] == 1 && on_bridge[idx[q]]) remove.push_back(idx[q]);
                    }
            }
            if (remove.empty()) {   // the weakest active edge of every violating node: first minimum in edge order (np.argmin)
                for (int side = 0; side < 2; ++side)
                    for (int v = 0; v < n; ++v) {
                        if ((side == 0 ? fo[v] : fi[v]) <= 3) continue;
                        const std::vector<int>& ptr = side == 0 ? out_ptr : in_ptr;
                        const std::vector<int>& idx = side == 0 ? out_idx : in_idx;
                        int best = -1;
                        for (int q = ptr[v]; q < ptr[v + 1]; ++q) {
                            const int k = idx[q];
                            if (p[k] == 1 && (best < 0 || probs[k] < probs[best])) best = k;
                        }
                        if (best >= 0) remove.push_back(best);
                    }
            }
            for (int k : remove) p[k] = 0;
            compact(p, a);
            flows(a);
            if (!violated()) return true;
        }
    }

    // the first label with more than four members, -1 if none
    int big_label(const std::vector<int>& lab_of) {
        int n_lab = 0;
        for (int v : lab_of) n_lab = std::max(n_lab, v + 1);
        count.assign(n_lab, 0);
        for (int v : lab_of) count[v]++;
        for (int c = 0; c < n_lab; ++c)
            if (count[c] > 4) return c;
        return -1;
    }

    // one removal round of utils.disjoint_big_clusters on (cur, a), in place: the weakest bridge of the frame, or -- with no bridge anywhere --
    // the weakest active edge touching label `lab`; EVERY edge with that probability goes (the reference zeroes inactive edges of that
    // probability too: they are 0 already).  false: nothing to remove.
    bool remove_weakest(Pred& cur, std::vector<int>& a, const std::vector<int>& lab_of, int lab) {
        bridge_set(a);
        float mn = 0.f;
        bool have = false;
        if (!bridge_list.empty()) {
            first_tab.reset(n);                                 // predicted_act_edges.index(bridge): the FIRST active edge with that (u, v)
            for (int k : a) first_tab.insert(eu[k], ev[k], k);
            for (size_t b = 0; b + 1 < bridge_list.size(); b += 2) {
                const int k = first_tab.get(bridge_list[b], bridge_list[b + 1]);
                if (k < 0) continue;                            // (cannot happen after pruning: both directions are active)
                if (!have || probs[k] < mn) mn = probs[k], have = true;
            }
        } else {
            for (int k : a)
                if (lab_of[eu[k]] == lab || lab_of[ev[k]] == lab)
                    if (!have || probs[k] < mn) mn = probs[k], have = true;
        }
        if (!have) return false;   // the reference would raise on an empty minimum; unreachable with a cluster of five
        for (int k : a)
            if (probs[k] == mn) cur[k] = 0;
        compact(cur, a);
        return true;
    }

    // utils.disjoint_big_clusters on (pred, a) with the labelling `ids` (all in / out): afterwards `pred` is the reference's RETURN value.
    // The reference modifies its argument in place until its first pruning makes a new object, and recurses once the big cluster is down to
    // four members -- dropping the recursive call's return value, so that of the recursion only its first in-place removal (on the caller's
    // current object) survives: that removal is all that is evaluated here.
    void split_big_clusters(Pred& pred, std::vector<int>& a) {
        const int lab = big_label(ids);
        if (lab < 0) return;
        for (;;) {
            if (!remove_weakest(pred, a, ids, lab)) return;
            cluster_ids(a, ids);
            int members = 0;
            for (int v : ids) members += v == lab;
            prune(pred, a);
            if (members <= 4) {
                const int lab2 = big_label(ids);                // the recursive call: its first removal round, in place, nothing else
                if (lab2 >= 0) (void)remove_weakest(pred, a, ids, lab2);
                return;
            }
        }
    }
};

static Solver& solver() {
    static thread_local Solver s;
    return s;
}

static int finalize_frame(const int64_t* src, const int64_t* dst, int64_t node_base, int64_t n_nodes, int64_t n_edges, const float* probs,
                          int64_t* predictions, int32_t switches, int32_t* labels_out, int32_t* n_clusters_out, int64_t* id_pred_out) {
    if (n_nodes < 0 || n_edges < 0 || n_nodes >= (1ll << 24) || n_edges >= (1ll << 30)) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges > 0 && (!src || !dst || !probs || !predictions)) return GNNCCA_ERR_INVALID_ARG;
    Solver& s = solver();
    if (!s.load(src, dst, node_base, n_nodes, n_edges, probs)) return GNNCCA_ERR_INVALID_ARG;
    Pred& pred = s.work;
    pred.assign(predictions, predictions + n_edges);
    std::vector<int>& act = s.act;
    act.clear();
    for (int k = 0; k < s.E; ++k) {
        if (pred[k] == 1)
            act.push_back(k);
        else if (pred[k] != 0)
            return GNNCCA_ERR_INVALID_ARG;   // thresholded predictions are 0 / 1 (inference.py:291)
    }
    const bool do_round = (switches & GNNCCA_POST_ROUNDING) != 0, do_prune = (switches & GNNCCA_POST_PRUNING) != 0,
               do_split = (switches & GNNCCA_POST_SPLITTING) != 0;
    if (do_prune) s.prune(pred, act);
    if (do_round) (void)s.rounding(pred, act);
    if (do_prune) s.prune(pred, act);
    int k = s.cluster_ids(act, s.ids);
    if (do_split) {
        s.split_big_clusters(pred, act);
        k = s.cluster_ids(act, s.ids);
    }
    for (int e = 0; e < s.E; ++e) predictions[e] = pred[e];
    if (id_pred_out)
        for (int v = 0; v < s.n; ++v) id_pred_out[v] = s.ids[v];
    if (labels_out) {   // the device chain's convention (post_cc_kernel): the smallest (batch-global) node id of the component
        std::vector<int>& smallest = s.count;
        smallest.assign(k, s.n);
        for (int v = 0; v < s.n; ++v) smallest[s.ids[v]] = std::min(smallest[s.ids[v]], v);
        for (int v = 0; v < s.n; ++v) labels_out[v] = (int32_t)(smallest[s.ids[v]] + node_base);
    }
    if (n_clusters_out) *n_clusters_out = k;
    return GNNCCA_OK;
}

// ---- the persistent pool ------------------------------------------------------------------------------------------------------------
struct Job {
    gnncca_post_batch b;
    hipEvent_t e_copy = nullptr;   // gnncca_post_pool_submit_copy's event (the pool's: returned to its free list by wait)
    std::vector<int32_t> flagged, k_new;
    std::atomic<int> next{0}, left{0}, status{GNNCCA_OK};
    int before = 0;
    bool done = false;
    double t_submit = 0, t_head = 0, t_event = 0, t_done = 0;   // microseconds on the steady clock (gnncca_post_pool_wait_timed)
    std::mutex m;
    std::condition_variable cv;
};

static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Task {
    std::shared_ptr<Job> job;   // (a queued or running task keeps its job alive: the waiter may collect the ticket while helpers are still leaving)
    bool head;
};

}  // namespace

struct gnncca_post_pool {
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv;
    std::deque<Task> tasks;
    std::unordered_map<int64_t, std::shared_ptr<Job>> jobs;
    int64_t next_ticket = 0;
    bool stop = false;
    std::atomic<int> queued{0};            // tasks in the queue (what a spinning thread polls without the mutex)
    std::atomic<bool> stop_flag{false};
    std::vector<hipEvent_t> free_events;   // recycled (creating and destroying events per batch cost microseconds of the caller's thread)

    void finish(Job* j) {
        {
            std::lock_guard<std::mutex> g(j->m);
            j->t_done = now_us();
            j->done = true;
        }
        j->cv.notify_all();
    }

    void frames_of(Job* j) {   // take flagged frames until none is left; the thread that finishes the last one closes the job
        const gnncca_post_batch& b = j->b;
        const int total = (int)j->flagged.size();
        for (int i = j->next.fetch_add(1); i < total; i = j->next.fetch_add(1)) {
            const int g = j->flagged[i];
            const int64_t v0 = b.node_ptr[g], v1 = b.node_ptr[g + 1], k0 = b.edge_ptr[g], k1 = b.edge_ptr[g + 1];
            const int st = finalize_frame(b.src + k0, b.dst + k0, v0, v1 - v0, k1 - k0, b.probs + k0, b.predictions + k0, b.switches,
                                          b.labels ? b.labels + v0 : nullptr, &j->k_new[i], nullptr);
            if (st != GNNCCA_OK) {
                int expected = GNNCCA_OK;
                j->status.compare_exchange_strong(expected, st);
            }
            if (j->left.fetch_sub(1) == 1) {
                if (b.n_clusters) {
                    int64_t total_k = *b.n_clusters - j->before;
                    for (int32_t q : j->k_new) total_k += q;
                    *b.n_clusters = (int32_t)total_k;
                }
                finish(j);
            }
        }
    }

    void head(const std::shared_ptr<Job>& jp) {
        Job* j = jp.get();
        gnncca_post_batch& b = j->b;
        j->t_head = now_us();
        if (b.ready_event) {
            (void)hipSetDevice(b.device);
            if (hipEventSynchronize(static_cast<hipEvent_t>(b.ready_event)) != hipSuccess) {
                j->status.store(GNNCCA_ERR_HIP);
                finish(j);
                return;
            }
        }
        j->t_event = now_us();
        const int want = ((b.switches & GNNCCA_POST_ROUNDING) ? GNNCCA_POST_TRIGGER_ROUNDING : 0) |
                         ((b.switches & GNNCCA_POST_SPLITTING) ? GNNCCA_POST_TRIGGER_SPLITTING : 0);
        for (int32_t g = 0; g < b.n_frames; ++g)
            if (b.triggers[g] & want) j->flagged.push_back(g);
        if (j->flagged.empty()) {
            finish(j);
            return;
        }
        j->k_new.assign(j->flagged.size(), 0);
        if (b.labels)   // clusters the device chain counted in the flagged frames: a component's label is its smallest node id
            for (int32_t g : j->flagged)
                for (int32_t v = b.node_ptr[g]; v < b.node_ptr[g + 1]; ++v) j->before += b.labels[v] == v;
        j->left.store((int)j->flagged.size());
        // helpers: one per `chunk` flagged frames, not one per thread -- waking a sleeping thread costs 50-100 us on the GPU boxes' hosts, a
        // frame 10 us: sixteen helpers for 58 frames spent 175 us, most of it waiting for each other to wake (tools/time_final_async.py)
        static const int chunk = gnncca::diag_env_int("GNNCCA_POOL_CHUNK", 12, 1, 1 << 20);
        const int helpers = std::min<int>(((int)j->flagged.size() + chunk - 1) / chunk, (int)threads.size()) - 1;
        if (helpers > 0) {
            {
                std::lock_guard<std::mutex> g(m);
                for (int h = 0; h < helpers; ++h) tasks.push_back(Task{jp, false});
                queued.fetch_add(helpers);
            }
            for (int h = 0; h < helpers; ++h) cv.notify_one();
        }
        frames_of(j);
    }

    void loop() {
        static const int spin_us = gnncca::diag_env_int("GNNCCA_POOL_SPIN_US", 60, 0, 100000);
        for (;;) {
            Task t;
            {
                // a thread that has just finished a task looks for the next one for a few tens of microseconds before it goes to sleep:
                // in a running pipeline the next batch's tasks arrive within that time, and the wake-up is what a job's latency is made of
                if (spin_us > 0 && queued.load(std::memory_order_relaxed) == 0) {
                    const double until = now_us() + spin_us;
                    while (queued.load(std::memory_order_relaxed) == 0 && !stop_flag.load(std::memory_order_relaxed) && now_us() < until) {
#if defined(__x86_64__)
                        __builtin_ia32_pause();
#endif
                    }
                }
                std::unique_lock<std::mutex> g(m);
                cv.wait(g, [&] { return stop || !tasks.empty(); });
                if (tasks.empty()) return;   // (stop, and nothing left to do)
                t = tasks.front();
                tasks.pop_front();
                queued.fetch_sub(1);
            }
            if (t.head)
                head(t.job);
            else
                frames_of(t.job.get());
        }
    }
};

extern "C" {

int gnncca_post_finalize_frame_host(const int64_t* src, const int64_t* dst, int64_t node_base, int64_t n_nodes, int64_t n_edges,
                                    const float* probs, int64_t* predictions, int32_t switches, int32_t* labels_out,
                                    int32_t* n_clusters_out, int64_t* id_pred_out) {
    return finalize_frame(src, dst, node_base, n_nodes, n_edges, probs, predictions, switches, labels_out, n_clusters_out, id_pred_out);
}

// The same for a list of frames of ONE batch (Batch.from_data_list layout: frame g owns nodes [node_ptr[g], node_ptr[g + 1]) and the contiguous
// edges [edge_ptr[g], edge_ptr[g + 1]); src / dst / probs / predictions / labels are the BATCH's arrays): frames[i] names a frame to finalize,
// clusters_out[i] receives its final cluster count; frames are independent, so they are dealt to up to `n_threads` host threads (0: one per
// hardware thread, at most 16).  Returns the first non-zero status of any frame.  (Synchronous, threads of its own; the pool below is the
// asynchronous form.)
int gnncca_post_finalize_frames_host(const int64_t* src, const int64_t* dst, const int32_t* node_ptr, const int32_t* edge_ptr,
                                     const int32_t* frames, int32_t n_listed, const float* probs, int64_t* predictions, int32_t switches,
                                     int32_t* labels, int32_t* clusters_out, int32_t n_threads) {
    if (n_listed < 0 || (n_listed > 0 && (!node_ptr || !edge_ptr || !frames || !clusters_out))) return GNNCCA_ERR_INVALID_ARG;
    if (n_listed == 0) return GNNCCA_OK;
    int nt = n_threads > 0 ? n_threads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    nt = std::min(nt, (int)((n_listed + 7) / 8));   // a thread is worth starting for eight frames or more (14 us each)
    std::atomic<int> next(0), status(GNNCCA_OK);
    auto work = [&]() {
        for (int i = next.fetch_add(1); i < n_listed; i = next.fetch_add(1)) {
            const int g = frames[i];
            const int64_t v0 = node_ptr[g], v1 = node_ptr[g + 1], k0 = edge_ptr[g], k1 = edge_ptr[g + 1];
            const int st = finalize_frame(src + k0, dst + k0, v0, v1 - v0, k1 - k0, probs + k0, predictions + k0, switches,
                                          labels ? labels + v0 : nullptr, clusters_out + i, nullptr);
            if (st != GNNCCA_OK) {
                int expected = GNNCCA_OK;
                status.compare_exchange_strong(expected, st);
            }
        }
    };
    if (nt <= 1) {
        work();
    } else {
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; ++t) pool.emplace_back(work);
        work();
        for (auto& t : pool) t.join();
    }
    return status.load();
}

gnncca_post_pool* gnncca_post_pool_create(int32_t n_threads) {
    int nt = n_threads > 0 ? n_threads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency() > 2 ? std::thread::hardware_concurrency() - 2 : 1u));
    nt = std::min(nt, 64);
    gnncca_post_pool* p = new (std::nothrow) gnncca_post_pool();
    if (!p) return nullptr;
    try {
        for (int t = 0; t < nt; ++t) p->threads.emplace_back([p] { p->loop(); });
    } catch (...) {
        gnncca_post_pool_destroy(p);
        return nullptr;
    }
    return p;
}

int32_t gnncca_post_pool_threads(const gnncca_post_pool* pool) { return pool ? (int32_t)pool->threads.size() : 0; }

void gnncca_post_pool_destroy(gnncca_post_pool* pool) {
    if (!pool) return;
    {
        std::lock_guard<std::mutex> g(pool->m);
        pool->stop = true;
        pool->stop_flag.store(true);
    }
    pool->cv.notify_all();
    for (auto& t : pool->threads)
        if (t.joinable()) t.join();   // (queued tasks are drained first: loop() leaves only on an empty queue)
    for (hipEvent_t e : pool->free_events) (void)hipEventDestroy(e);
    for (auto& kv : pool->jobs) {   // (tickets nobody collected)
        if (kv.second->e_copy) (void)hipEventDestroy(kv.second->e_copy);
    }
    delete pool;
}

static bool batch_ok(const gnncca_post_batch* batch) {
    if (!batch || batch->n_frames < 0) return false;
    if (batch->n_clusters && !batch->labels) return false;   // the final count is the device chain's count corrected by the flagged frames' labels
    return batch->n_frames == 0 || (batch->node_ptr && batch->edge_ptr && batch->triggers && batch->src && batch->dst && batch->probs && batch->predictions);
}

static int64_t enqueue(gnncca_post_pool* pool, std::shared_ptr<Job> j) {
    int64_t ticket;
    j->t_submit = now_us();
    {
        std::lock_guard<std::mutex> g(pool->m);
        ticket = pool->next_ticket++;
        pool->tasks.push_back(Task{j, true});
        pool->queued.fetch_add(1);
        pool->jobs.emplace(ticket, std::move(j));
    }
    pool->cv.notify_one();
    return ticket;
}

// submit for results that still sit in DEVICE memory: the D2H copy of `nbytes` from device_src to host_dst (pinned) is enqueued on `stream`
// itself -- the stream the batch's chain was enqueued on -- with the event the job waits for right behind it.  One call, no synchronisation;
// `batch` points into host_dst.  (The first version copied on a stream of the pool's own behind an event: one event and one cross-stream wait
// more per batch, and in a process that already uses several streams the new stream shares a hardware queue with one of them -- this device
// maps streams onto four queues -- so the copy queued up behind LATER batches' kernels: 0.15 ms per batch in a fresh process, 0.3-0.4 ms
// inside bench.py.  The copy is 0.6 MB, ~15 us of a stream whose chain is host-bound.)
int64_t gnncca_post_pool_submit_copy(gnncca_post_pool* pool, const gnncca_post_batch* batch, const void* device_src, void* host_dst,
                                     size_t nbytes, int32_t device, gnncca_stream_t stream) {
    if (!pool || !batch_ok(batch) || !device_src || !host_dst || nbytes == 0 || device < 0) return -(int64_t)GNNCCA_ERR_INVALID_ARG;
    std::shared_ptr<Job> j(new (std::nothrow) Job());
    if (!j) return -(int64_t)GNNCCA_ERR_INVALID_ARG;
    j->b = *batch;
    {
        std::lock_guard<std::mutex> g(pool->m);
        if (!pool->free_events.empty()) j->e_copy = pool->free_events.back(), pool->free_events.pop_back();
    }
    // (e_copy is what a pool thread waits on: an event without hipEventBlockingSync, so that wait is a spin, not a sleep)
    if (!j->e_copy && hipEventCreateWithFlags(&j->e_copy, hipEventDisableTiming) != hipSuccess)
        return -(int64_t)GNNCCA_ERR_HIP;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemcpyAsync(host_dst, device_src, nbytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipEventRecord(j->e_copy, st) != hipSuccess) {
        (void)hipEventDestroy(j->e_copy);
        return -(int64_t)GNNCCA_ERR_HIP;
    }
    j->b.ready_event = j->e_copy;
    j->b.device = device;
    return enqueue(pool, std::move(j));
}

int64_t gnncca_post_pool_submit(gnncca_post_pool* pool, const gnncca_post_batch* batch) {
    if (!pool || !batch_ok(batch)) return -(int64_t)GNNCCA_ERR_INVALID_ARG;
    std::shared_ptr<Job> j(new (std::nothrow) Job());
    if (!j) return -(int64_t)GNNCCA_ERR_INVALID_ARG;
    j->b = *batch;
    return enqueue(pool, std::move(j));
}

int gnncca_post_pool_wait(gnncca_post_pool* pool, int64_t ticket, int32_t* frames_out, int32_t* n_frames_out) {
    return gnncca_post_pool_wait_timed(pool, ticket, frames_out, n_frames_out, nullptr);
}

// diagnostics: the same, plus the job's life in microseconds -- times_us_out[0..3] = submit -> a pool thread picked it up, -> its event had
// completed (the D2H copy behind the GPU chain), -> the last frame was final, -> this call returned
int gnncca_post_pool_wait_timed(gnncca_post_pool* pool, int64_t ticket, int32_t* frames_out, int32_t* n_frames_out, double* times_us_out) {
    if (!pool) return GNNCCA_ERR_INVALID_ARG;
    std::shared_ptr<Job> j;
    {
        std::lock_guard<std::mutex> g(pool->m);
        auto q = pool->jobs.find(ticket);
        if (q == pool->jobs.end()) return GNNCCA_ERR_INVALID_ARG;
        j = q->second;
    }
    {
        std::unique_lock<std::mutex> g(j->m);
        j->cv.wait(g, [&] { return j->done; });
    }
    const int st = j->status.load();
    if (times_us_out) {
        times_us_out[0] = j->t_head - j->t_submit, times_us_out[1] = j->t_event - j->t_head;
        times_us_out[2] = j->t_done - j->t_event, times_us_out[3] = now_us() - j->t_done;
    }
    if (n_frames_out) *n_frames_out = (int32_t)j->flagged.size();
    if (frames_out)
        for (size_t i = 0; i < j->flagged.size(); ++i) frames_out[i] = j->flagged[i];
    {
        std::lock_guard<std::mutex> g(pool->m);
        if (j->e_copy) pool->free_events.push_back(j->e_copy), j->e_copy = nullptr;
        pool->jobs.erase(ticket);
    }
    return st;
}

}  // extern "C"
