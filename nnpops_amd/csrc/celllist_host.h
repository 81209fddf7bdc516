// celllist_host.h -- the host-side owner of one cell grid (celllist.h): the sizes of its arrays, their allocation and release,
// the growth of the bins and the read-back of the grid.  The stateful handles (ani.hip, cfconv.hip) hold a CellList; the
// stateless getNeighborPairs op carves the same arrays, by the same sizes, out of its caller's workspace.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "celllist.h"
#include "host_common.h"

namespace nnpops {

// device grid -> the eight words of grid_words (what the three read_grid entry points do)
inline int read_grid_words(const CellGrid* d_grid, hipStream_t stream, int32_t* out) {
    CellGrid g;
    NNPOPS_HIP_TRY(hipMemcpyAsync(&g, d_grid, sizeof(CellGrid), hipMemcpyDeviceToHost, stream));
    NNPOPS_HIP_TRY(hipStreamSynchronize(stream));
    grid_words(g, out);
    return NNPOPS_OK;
}

struct CellList : CellBuffers {
    static int cells_for(int N) { return N + 4096; }           // the cap on the cell count that decide_grid is given
    static size_t tile_total_len(int max_cells) { return (size_t)max_cells / kScanTile + 2; }

    // Every array of the grid with its length, in the one place that allocate() and release() both walk.
    // binned: the histogram and bins of the two-kernel build; tiled_scan: the partial sums of the tiled scan.
    template <typename F>
    int each_array(size_t n, bool binned, bool tiled_scan, F&& f) {
        int rc = NNPOPS_OK;
        auto visit = [&](auto*& p, size_t len) { if (rc == NNPOPS_OK) rc = f(p, len); };
        visit(grid, 1);
        visit(cell_count, (size_t)max_cells);
        visit(cell_start, (size_t)max_cells + 1);
        visit(atom_cell, n);
        visit(atom_rank, n);
        visit(unsorted_atom, n);
        visit(sorted_atom, n);
        visit(sorted_pos, n);
        visit(sorted_cell, n);
        if (binned) { visit(hist, (size_t)kHistWords); visit(bins, (size_t)kBinnedCells * bin_cap); }
        if (tiled_scan) visit(tile_total, tile_total_len(max_cells));
        return rc;
    }

    // tiled_scan = false: no tile_total, and launch_cell_build scans with one block whatever the size of the grid
    int allocate(int N, bool periodic, bool tiled_scan) {
        max_cells = cells_for(N);
        bin_cap = 64;
        if (const char* e = std::getenv("NNPOPS_CELL_BIN_CAP")) bin_cap = std::max(4, std::atoi(e) & ~3);   // tests: force growth
        const bool binned = periodic && N <= kBinnedAtoms;
        int rc = each_array((size_t)N, binned, tiled_scan, [](auto*& p, size_t len) { return dev_alloc(&p, len); });
        if (rc != NNPOPS_OK) return rc;
        if (hipMemset(grid, 0, sizeof(CellGrid)) != hipSuccess) return fail(NNPOPS_ERR_HIP, "memset failed");      // (bin_overflow: the one-launch build never clears it)
        if (binned && hipMemset(hist, 0, sizeof(int) * kHistWords) != hipSuccess) return fail(NNPOPS_ERR_HIP, "memset failed");
        return NNPOPS_OK;
    }

    // (also after an allocate() that failed half way: an array that was never allocated is null)
    void release() {
        each_array(0, true, true, [](auto*& p, size_t) { dev_free(p); return (int)NNPOPS_OK; });
    }

    // a bin overflowed (kGridBinOverflow): twice the ids per cell; the new capacity is bin_cap
    int grow_bins(int* old_cap) {
        *old_cap = bin_cap;
        bin_cap *= 2;
        dev_free(bins);
        return dev_alloc(&bins, (size_t)kBinnedCells * bin_cap);
    }

    int read_words(hipStream_t stream, int32_t* out) const { return read_grid_words(grid, stream, out); }
};

}  // namespace nnpops
