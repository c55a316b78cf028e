// The Dulmage-Mendelsohn decomposition (spasm_dm.c:90), strongly connected components (spasm_scc.c:14), the maximum matching's
// entry points (spasm_matching.c:103) and the permutations they need (spasm_permutation.c:49-99).
//
// The matching and the two alternating searches of the coarse decomposition run on the device (matching.hip).  The sets are
// collected here in the reference's order (spasm_dm.c:63-87): q = C0 | C1 | C2 | C3, p = R1 | R2 | R3 | R0, inside every set the
// columns in increasing index with their matched rows beside them, R0 in increasing index.  The strongly connected components
// of S are computed here too, by an iterative Tarjan, linear in the size of S: a level-synchronous device SCC and the
// topological order of its condensation take one step per link of the longest chain of the DAG (a triangular S with 10^6
// trivial blocks: 10^6 launches), where the host needs milliseconds.  DESIGN.md section 11.
#include <algorithm>
#include <mutex>
#include <vector>

#include "common.h"
#include "dm.h"

namespace sh {

namespace {

constexpr int DM_STATS = 13;
std::mutex dm_stats_mutex;
double dm_last[DM_STATS];

struct spasm_dm *dm_alloc(int n, int m)
{
	struct spasm_dm *P = (struct spasm_dm *) xmalloc(sizeof(*P));
	P->p = (int *) xmalloc((int64_t) n * 4);
	P->q = (int *) xmalloc((int64_t) m * 4);
	P->r = (int *) xmalloc((int64_t) (n + 6) * 4);
	P->c = (int *) xmalloc((int64_t) (m + 6) * 4);
	P->nb = 0;
	for (int t = 0; t < 5; t++) {
		P->rr[t] = 0;
		P->cc[t] = 0;
	}
	return P;
}

// Tarjan's strongly connected components of the digraph on 0 .. s-1 (arcs v -> aj[ap[v] .. ap[v+1])), without recursion.
// order receives the vertices block after block, bounds the nb + 1 block boundaries; the blocks come out in topological order
// (every arc goes from a block to itself or to a later one).  Returns nb.
int tarjan(int s, const int64_t *ap, const int *aj, int *order, std::vector<int> &bounds)
{
	std::vector<int> index((size_t) s, -1), low((size_t) s), stack, calls;
	std::vector<int64_t> next((size_t) s);
	std::vector<char> on_stack((size_t) s, 0);
	stack.reserve((size_t) s);
	int counter = 0, placed = s;                   // blocks are placed from the end: Tarjan finds the sinks first
	std::vector<int> rev_bounds{s};
	for (int v0 = 0; v0 < s; v0++) {
		if (index[v0] >= 0)
			continue;
		auto open = [&](int v) {
			index[v] = low[v] = counter++;
			next[v] = ap[v];
			stack.push_back(v);
			on_stack[v] = 1;
			calls.push_back(v);
		};
		open(v0);
		while (!calls.empty()) {
			const int v = calls.back();
			if (next[v] < ap[v + 1]) {
				const int w = aj[next[v]++];
				if (index[w] < 0)
					open(w);
				else if (on_stack[w])
					low[v] = std::min(low[v], index[w]);
				continue;
			}
			calls.pop_back();
			if (!calls.empty())
				low[calls.back()] = std::min(low[calls.back()], low[v]);
			if (low[v] != index[v])
				continue;
			// v is the root of a block: its vertices are on the stack above it
			size_t top = stack.size();
			while (stack[top - 1] != v)
				top--;
			top--;
			const int size = (int) (stack.size() - top);
			placed -= size;
			for (int t = 0; t < size; t++) {
				const int w = stack[top + t];
				order[placed + t] = w;
				on_stack[w] = 0;
			}
			stack.resize(top);
			rev_bounds.push_back(placed);
		}
	}
	bounds.assign(rev_bounds.rbegin(), rev_bounds.rend());
	return (int) bounds.size() - 1;
}

// the sets of the coarse decomposition in the reference's layout (spasm_dm.c:63-87)
void collect_coarse(int n, int m, const int *jmatch, const int *imatch, const std::vector<char> &r1, const std::vector<char> &c3,
                    struct spasm_dm *P, const char *who)
{
	// column marks: 0 C0, 1 C1, 2 C2, 3 C3
	std::vector<char> cm((size_t) m);
	for (int j = 0; j < m; j++) {
		const int i = imatch[j];
		if (i < 0)
			cm[j] = 0;
		else if (c3[j])
			cm[j] = 3;
		else if (r1[i])
			cm[j] = 1;
		else
			cm[j] = 2;
		if (i >= 0 && c3[j] && r1[i])
			die("%s: row %d is reachable from both sides (the matching is not maximum)", who, i);
	}
	int kc = 0, kr = 0;
	P->cc[0] = 0;
	P->rr[0] = 0;
	for (int j = 0; j < m; j++)
		if (cm[j] == 0)
			P->q[kc++] = j;
	P->cc[1] = kc;
	for (int set = 1; set <= 3; set++) {
		for (int j = 0; j < m; j++)
			if (cm[j] == set) {
				P->p[kr++] = imatch[j];
				P->q[kc++] = j;
			}
		P->cc[set + 1] = kc;
		P->rr[set] = kr;
	}
	for (int i = 0; i < n; i++)
		if (jmatch[i] < 0)
			P->p[kr++] = i;
	P->rr[4] = kr;
	if (kr != n || kc != m)
		die("%s: the coarse decomposition covers %d of %d rows, %d of %d columns", who, kr, n, kc, m);
}

// fine decomposition: the blocks of S = A(R2, C2) (its matched pairs on the diagonal), H before them, V after them
void fine_blocks(const struct spasm_csr *A, struct spasm_dm *P)
{
	const int n = A->n, m = A->m, r1 = P->rr[1], c2 = P->cc[2], s = P->rr[2] - P->rr[1];
	std::vector<int> bounds{0};
	if (s > 0) {
		std::vector<int> col_of((size_t) m, -1);       // column -> its place in C2
		for (int t = 0; t < s; t++)
			col_of[P->q[c2 + t]] = t;
		std::vector<int64_t> sp((size_t) s + 1, 0);
		std::vector<int> sj;
		for (int t = 0; t < s; t++) {
			const int i = P->p[r1 + t];
			for (int64_t px = A->p[i]; px < A->p[i + 1]; px++) {
				const int u = col_of[A->j[px]];
				if (u >= 0)
					sj.push_back(u);
			}
			sp[t + 1] = (int64_t) sj.size();
		}
		std::vector<int> order((size_t) s);
		tarjan(s, sp.data(), sj.data(), order.data(), bounds);
		std::vector<int> rows(P->p + r1, P->p + r1 + s), cols(P->q + c2, P->q + c2 + s);
		for (int k = 0; k < s; k++) {
			P->p[r1 + k] = rows[order[k]];
			P->q[c2 + k] = cols[order[k]];
		}
	}
	const int n_scc = (int) bounds.size() - 1;
	P->r[0] = 0;
	P->c[0] = 0;
	for (int b = 0; b <= n_scc; b++) {
		P->r[b + 1] = r1 + bounds[b];
		P->c[b + 1] = c2 + bounds[b];
	}
	P->r[n_scc + 2] = n;
	P->c[n_scc + 2] = m;
	P->nb = n_scc + 2;
}

void record(const DmMatchStats &St, double coarse_ms, double fine_ms, double total_ms, int nb)
{
	std::lock_guard<std::mutex> guard(dm_stats_mutex);
	const double v[DM_STATS] = {St.upload_ms, St.greedy_ms, St.phases_ms, St.reach_ms, coarse_ms, fine_ms, total_ms,
	                            (double) St.greedy_size, (double) St.phases, (double) St.levels, (double) St.small_levels,
	                            (double) St.size, (double) nb};
	std::copy(v, v + DM_STATS, dm_last);
}

}  // namespace

}  // namespace sh

using namespace sh;

extern "C" {

struct spasm_dm *spasm_hip_dm_alloc(int n, int m)
{
	if (n < 0 || m < 0)
		die("spasm_hip_dm_alloc: %d x %d", n, m);
	return dm_alloc(n, m);
}

void spasm_hip_dm_free(struct spasm_dm *P)
{
	if (P == nullptr)
		return;
	free(P->p);
	free(P->q);
	free(P->r);
	free(P->c);
	free(P);
}

int spasm_hip_maximum_matching(const struct spasm_csr *A, int *jmatch, int *imatch)
{
	const char *who = "spasm_hip_maximum_matching";
	check_host_csr(A, who, true);
	const double t0 = wtime();
	DmMatchStats St;
	const int k = dm_match(A, who, jmatch, imatch, nullptr, nullptr, &St);
	record(St, 0, 0, (wtime() - t0) * 1e3, 0);
	if (verbose() >= 2)
		logmsg("[matching] %d x %d: size %d (greedy %d, %d phases, %lld levels) [%.3f s]\n", A->n, A->m, k, St.greedy_size, St.phases,
		       St.levels, wtime() - t0);
	return k;
}

int spasm_hip_structural_rank(const struct spasm_csr *A)
{
	check_host_csr(A, "spasm_hip_structural_rank", true);
	std::vector<int> jmatch((size_t) std::max(A->n, 1)), imatch((size_t) std::max(A->m, 1));
	return spasm_hip_maximum_matching(A, jmatch.data(), imatch.data());
}

struct spasm_dm *spasm_hip_dulmage_mendelsohn(const struct spasm_csr *A)
{
	const char *who = "spasm_hip_dulmage_mendelsohn";
	check_host_csr(A, who, true);
	const double t0 = wtime();
	const int n = A->n, m = A->m;
	std::vector<int> jmatch((size_t) std::max(n, 1)), imatch((size_t) std::max(m, 1));
	std::vector<char> r1, c3;
	DmMatchStats St;
	dm_match(A, who, jmatch.data(), imatch.data(), &r1, &c3, &St);
	const double t1 = wtime();
	struct spasm_dm *P = dm_alloc(n, m);
	collect_coarse(n, m, jmatch.data(), imatch.data(), r1, c3, P, who);
	const double t2 = wtime();
	fine_blocks(A, P);
	const double t3 = wtime();
	record(St, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3, P->nb);
	if (verbose() >= 2)
		logmsg("[dm] %d x %d: structural rank %d, S %d x %d in %d blocks [matching %.3f s, coarse %.3f s, SCC %.3f s]\n", n, m, St.size,
		       P->rr[2] - P->rr[1], P->cc[3] - P->cc[2], P->nb - 2, t1 - t0, t2 - t1, t3 - t2);
	return P;
}

struct spasm_dm *spasm_hip_strongly_connected_components(const struct spasm_csr *A)
{
	const char *who = "spasm_hip_strongly_connected_components";
	check_host_csr(A, who, true);
	if (A->n != A->m)
		die("%s: A is %d x %d, not square", who, A->n, A->m);
	const int n = A->n;
	struct spasm_dm *P = dm_alloc(n, n);
	std::vector<int> bounds;
	const int64_t zero = 0;
	P->nb = tarjan(n, n > 0 ? A->p : &zero, A->j, P->p, bounds);
	std::copy(P->p, P->p + n, P->q);
	std::copy(bounds.begin(), bounds.end(), P->r);
	std::copy(bounds.begin(), bounds.end(), P->c);
	return P;
}

int *spasm_hip_pinv(const int *p, int n)
{
	if (p == nullptr)
		return nullptr;
	int *pinv = (int *) xmalloc((int64_t) n * 4);
	for (int k = 0; k < n; k++)
		pinv[k] = -1;
	for (int k = 0; k < n; k++) {
		if (p[k] < 0 || p[k] >= n || pinv[p[k]] >= 0)
			die("spasm_hip_pinv: the vector is not a permutation of 0 .. %d (entry %d)", n - 1, k);
		pinv[p[k]] = k;
	}
	return pinv;
}

struct spasm_csr *spasm_hip_permute(const struct spasm_csr *A, const int *p, const int *qinv, int with_values)
{
	check_host_csr(A, "spasm_hip_permute", true);
	const int n = A->n, m = A->m;
	const int64_t nnz = n > 0 ? A->p[n] : 0;
	struct spasm_csr *C = spasm_hip_csr_alloc(n, m, std::max<int64_t>(nnz, 1), A->field->p, with_values && A->x != nullptr);
	int64_t at = 0;
	for (int i = 0; i < n; i++) {
		C->p[i] = at;
		const int src = p != nullptr ? p[i] : i;
		if (src < 0 || src >= n)
			die("spasm_hip_permute: p[%d] = %d lies outside [0, %d)", i, src, n);
		for (int64_t px = A->p[src]; px < A->p[src + 1]; px++) {
			const int j = A->j[px];
			C->j[at] = qinv != nullptr ? qinv[j] : j;
			if (C->x != nullptr)
				C->x[at] = A->x[px];
			at++;
		}
	}
	C->p[n] = at;
	return C;
}

int spasm_hip_dm_stats(double *out, int count)
{
	std::lock_guard<std::mutex> guard(dm_stats_mutex);
	for (int t = 0; t < std::min(count, DM_STATS); t++)
		out[t] = dm_last[t];
	return DM_STATS;
}

}  // extern "C"
