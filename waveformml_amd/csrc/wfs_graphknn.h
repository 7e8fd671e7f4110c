// wfs_graphknn.h -- the neighbour selection of GraphNet's knn_graph (reference src/models/GraphNet.py:232 ->
// torch_cluster's brute-force kernel, RESTATED: torch_cluster is not available to hold it to), one function for the host
// entry point and the device kernel alike.
//
// Rows are int32 (x, y, event), grouped by event.  The candidates of row i are the other rows of its event's run (the row
// itself too with `self_loop`, at distance 0, and then `k` counts it); the distance is the squared integer distance on
// (x, y); the `k` smallest are kept, AMONG EQUAL DISTANCES THE LOWER ROW INDEX WINS: candidates are walked in row order and
// one moves in front of the kept entries that are strictly farther only.  The list comes out ordered by (distance, row).
// The row itself is left out by its INDEX, not by its distance: a duplicate segment of the same event is an ordinary
// neighbour at distance 0.
#pragma once
#include <stdint.h>

#define WFS_GRAPH_KMAX 8              // neighbours per row the tables hold
// CONTRACT: an event's run of rows is at most this long (a detector event: <= 154).  A row looks no further than this to
// either side, so that a batch that breaks the contract costs bounded time and no access leaves the arrays; but rows
// of a longer run then see different windows of it: their lists are not the k nearest of the event and the reverse
// lists (k_graph_rev) are incomplete.  Such a batch is outside what the tables are defined for.
#define WFS_GRAPH_EVENT_WINDOW 1024

// [first, last) of the run of rows that share row i's event number, among the first `nv` rows
__host__ __device__ inline void graph_event_run(const int32_t *coords, long long nv, long long i, long long *first,
                                                long long *last) {
    const int32_t e = coords[3 * i + 2];
    long long a = i, b = i + 1;          // the same reach both ways: first >= i - WINDOW, last (exclusive) <= i + WINDOW + 1
    while (a > 0 && i - a < WFS_GRAPH_EVENT_WINDOW && coords[3 * (a - 1) + 2] == e) --a;
    while (b < nv && b - i <= WFS_GRAPH_EVENT_WINDOW && coords[3 * b + 2] == e) ++b;
    *first = a;
    *last = b;
}

// out[0 .. deg) = the neighbours of row i among rows [first, last); returns deg <= k <= WFS_GRAPH_KMAX
__host__ __device__ inline int graph_knn_select(const int32_t *coords, long long first, long long last, long long i, int k,
                                                int self_loop, int32_t *out) {
    long long dist[WFS_GRAPH_KMAX];
    int n = 0;
    const long long xi = coords[3 * i], yi = coords[3 * i + 1];
    for (long long j = first; j < last; ++j) {
        if (j == i && !self_loop) continue;
        const long long dx = coords[3 * j] - xi, dy = coords[3 * j + 1] - yi;
        const long long d = dx * dx + dy * dy;
        int p = n;                                   // where the candidate lands: behind every entry that is not farther
        while (p > 0 && dist[p - 1] > d) --p;
        if (p >= k) continue;
        const int top = n < k ? n : k - 1;           // entries [p, top) move one place back (the last one drops out)
        for (int q = top; q > p; --q) {
            dist[q] = dist[q - 1];
            out[q] = out[q - 1];
        }
        dist[p] = d;
        out[p] = (int32_t)j;
        if (n < k) ++n;
    }
    return n;
}
