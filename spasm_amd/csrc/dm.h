// Maximum matching and the reachability sets of the coarse Dulmage-Mendelsohn decomposition on the device (matching.hip); the
// decomposition itself, the strongly connected components and the permutations are host code (host_dm.cpp).
#pragma once

#include <vector>

#include "common.h"

namespace sh {

// what one call of dm_match did (spasm_hip_dm_stats reports it beside the host stages)
struct DmMatchStats {
	double upload_ms = 0;        // A up, its column-major pattern built
	double greedy_ms = 0;
	double phases_ms = 0;        // augmenting phases
	double reach_ms = 0;         // the two alternating searches of the coarse decomposition, their download
	int greedy_size = 0;
	int phases = 0;              // augmenting phases, the last one (which finds nothing) included
	long long levels = 0;        // BFS levels of all phases and of the two searches
	long long small_levels = 0;  // ... of them run inside one workgroup
	int size = 0;
};

// A maximum matching of the pattern of A (n x m): jmatch[i] the column of row i, imatch[j] the row of column j, or -1; the
// size is returned.  With reach != nullptr also the coarse sets: row_r1[i] = 1 for the rows reachable by alternating paths from
// the unmatched columns (R1), col_c3[j] = 1 for the columns reachable from the unmatched rows (C3).  Dies on malformed input,
// without a device, or when a device search passes its bound.
int dm_match(const struct spasm_csr *A, const char *who, int *jmatch, int *imatch, std::vector<char> *row_r1, std::vector<char> *col_c3,
             DmMatchStats *stats);

}  // namespace sh
