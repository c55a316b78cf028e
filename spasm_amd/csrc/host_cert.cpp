// Rank certificates and factorization checks (replace spasm_certificate.c:21-270), host code over two GPU pieces: the solves
// of spasm_hip_gesv (solve.hip) and the products x.A of spmv.hip.
//
// Eberly's interactive certificate ("A New Interactive Certificate for Matrix Rank", 2015), as the reference builds it: the
// challenge is drawn from the SHA-256 generator seeded with the hash of the input file (prng.h, the reference's stream), r
// values for the pivot columns then one value per non-pivotal row.  The certificate holds the pivot rows i, the pivot columns
// j, and on the pivot rows the solutions x (x.A = alpha on the columns j) and y (y.A = 0 once the non-pivotal rows get their
// challenge values).  Both right-hand sides are solved in one gesv call; gesv is bit-identical to the reference's spasm_solve
// row by row, so the certificate is bit-identical to the reference's on the same factorization.  Verification repeats the
// reference's checks in its order; its two products x.A are one k = 2 call.
#include <cinttypes>
#include <vector>

#include "common.h"
#include "prng.h"
#include "xa.h"

using namespace sh;

namespace {

constexpr spasm_ZZp BOT = 0x7fffffff;       // "not set yet" (spasm_certificate.c:74, :141)

// the dense rows of a gesv result X (X->n x n)
std::vector<spasm_ZZp> dense_rows(const struct spasm_csr *X, int n)
{
	std::vector<spasm_ZZp> D((size_t) X->n * n, 0);
	for (int t = 0; t < X->n; t++)
		for (int64_t px = X->p[t]; px < X->p[t + 1]; px++)
			D[(size_t) t * n + X->j[px]] = X->x[px];
	return D;
}

void *xcalloc(int64_t count, int64_t size)
{
	void *q = std::calloc((size_t) std::max<int64_t>(count, 1), (size_t) size);
	if (q == nullptr)
		die("calloc failed (%lld x %lld bytes)", (long long) count, (long long) size);
	return q;
}

}  // namespace

extern "C" {

// the first `count` values of the stream spasm_prng_seed(seed, prime, seq) draws (exported for the tests)
void spasm_hip_debug_prng_hash(const u8 *seed, i64 prime, uint32_t seq, int count, spasm_ZZp *out)
{
	Prng g;
	g.seed_hash(seed, prime, seq);
	for (int i = 0; i < count; i++)
		out[i] = g.next_zp();
}

struct spasm_rank_certificate *spasm_hip_certificate_rank_create(const struct spasm_csr *A, const u8 *hash, const struct spasm_lu *fact)
{
	if (A == nullptr || hash == nullptr || fact == nullptr)
		die("spasm_hip_certificate_rank_create: NULL argument");
	if (fact->L == nullptr)
		die("spasm_hip_certificate_rank_create: fact->L is NULL (echelonize with opts->L = 1)");
	const struct spasm_csr *U = fact->U, *L = fact->L;
	const int n = L->n, m = U->m, r = U->n;
	const i64 prime = A->field->p;
	if (U->field->p != prime || L->field->p != prime)
		die("spasm_hip_certificate_rank_create: A is mod %lld, U mod %lld, L mod %lld", (long long) prime, (long long) U->field->p,
		    (long long) L->field->p);
	if (A->n != n || A->m != m)
		die("spasm_hip_certificate_rank_create: A is %d x %d, the factorization %d x %d", A->n, A->m, n, m);

	struct spasm_rank_certificate *proof = (struct spasm_rank_certificate *) xmalloc(sizeof(*proof));
	proof->r = r;
	std::memcpy(proof->hash, hash, 32);
	proof->prime = prime;
	int *ii = (int *) xcalloc(r, sizeof(int));
	int *jj = (int *) xcalloc(r, sizeof(int));
	spasm_ZZp *xx = (spasm_ZZp *) xcalloc(r, sizeof(spasm_ZZp));
	spasm_ZZp *yy = (spasm_ZZp *) xcalloc(r, sizeof(spasm_ZZp));
	proof->i = ii;
	proof->j = jj;
	proof->x = xx;
	proof->y = yy;

	// the positions of the pivots: rows of L (fact->p), columns of U by increasing index
	for (int k = 0; k < r; k++) {
		ii[k] = fact->p[k];
		if (ii[k] < 0 || ii[k] >= n)
			die("spasm_hip_certificate_rank_create: pivot %d sits on row %d of %d", k, ii[k], n);
	}
	int k = 0;
	for (int j = 0; j < m; j++)
		if (fact->qinv[j] >= 0) {
			if (k == r)
				die("spasm_hip_certificate_rank_create: more pivot columns than the rank %d", r);
			jj[k++] = j;
		}
	if (k != r)
		die("spasm_hip_certificate_rank_create: %d pivot columns, rank %d", k, r);

	// the challenge: r values on the pivot columns (first right-hand side), then minus one value per non-pivotal row, whose
	// product with A is the second right-hand side
	Prng g;
	g.seed_hash(hash, prime, 0);
	struct spasm_csr *B = spasm_hip_csr_alloc(2, m, std::max<int64_t>((int64_t) r + m, 1), prime, true);
	B->p[0] = 0;
	for (int t = 0; t < r; t++) {
		B->j[t] = jj[t];
		B->x[t] = g.next_zp();
	}
	B->p[1] = r;
	std::vector<spasm_ZZp> x((size_t) n, BOT), y((size_t) m, 0);
	for (int t = 0; t < r; t++)
		x[ii[t]] = 0;
	for (int i = 0; i < n; i++)
		if (x[i] == BOT)
			x[i] = -g.next_zp();
	spasm_hip_xApy_batch(A, 1, x.data(), y.data());
	int64_t w = r;
	for (int j = 0; j < m; j++)
		if (y[j] != 0) {
			B->j[w] = j;
			B->x[w] = y[j];
			w += 1;
		}
	B->p[2] = w;

	struct spasm_csr *X = spasm_hip_gesv(fact, B, nullptr);
	const std::vector<spasm_ZZp> D = dense_rows(X, n);
	for (int t = 0; t < r; t++) {
		xx[t] = D[ii[t]];
		yy[t] = D[(size_t) n + ii[t]];
	}
	spasm_hip_csr_free(X);
	spasm_hip_csr_free(B);
	return proof;
}

bool spasm_hip_certificate_rank_verify(const struct spasm_csr *A, const u8 *hash, const struct spasm_rank_certificate *proof)
{
	if (A == nullptr || hash == nullptr || proof == nullptr)
		die("spasm_hip_certificate_rank_verify: NULL argument");
	const int n = A->n, m = A->m, r = proof->r;
	for (int i = 0; i < 32; i++)
		if (hash[i] != proof->hash[i])
			return false;
	if (A->field->p != proof->prime)
		return false;
	for (int k = 0; k < r; k++) {
		if (proof->i[k] < 0 || proof->i[k] >= n)
			return false;
		if (proof->j[k] < 0 || proof->j[k] >= m)
			return false;
	}

	Prng g;
	g.seed_hash(proof->hash, proof->prime, 0);
	// the two vectors of the reference's two products: x on the pivot rows, then y completed by the challenge
	std::vector<spasm_ZZp> X((size_t) 2 * n, 0), Y((size_t) 2 * m, 0);
	spasm_ZZp *x0 = X.data(), *x1 = X.data() + n;
	for (int k = 0; k < r; k++)
		x0[proof->i[k]] = proof->x[k];
	std::vector<spasm_ZZp> alpha((size_t) std::max(r, 0));
	for (int k = 0; k < r; k++)
		alpha[k] = g.next_zp();
	for (int i = 0; i < n; i++)
		x1[i] = BOT;
	for (int k = 0; k < r; k++)
		x1[proof->i[k]] = proof->y[k];
	for (int i = 0; i < n; i++)
		if (x1[i] == BOT)
			x1[i] = g.next_zp();
	spasm_hip_xApy_batch(A, 2, X.data(), Y.data());
	bool correct = true;
	for (int k = 0; k < r; k++)
		if (Y[proof->j[k]] != alpha[k])
			correct = false;
	for (int j = 0; j < m; j++)
		if (Y[(size_t) m + j] != 0)
			correct = false;
	return correct;
}

// spasm_factorization_verify (spasm_certificate.c:165-219) for `count` seeds at once: x = one random value per pivotal row
// (spasm_prng_seed_simple(prime, seed, 0)), then x.A == (x.L).U?  Three k = count products, over A, L and U.
void spasm_hip_factorization_verify_batch(const struct spasm_csr *A, const struct spasm_lu *fact, int count, const u64 *seeds, bool *correct)
{
	if (A == nullptr || fact == nullptr || (count > 0 && (seeds == nullptr || correct == nullptr)))
		die("spasm_hip_factorization_verify: NULL argument");
	if (fact->L == nullptr)
		die("spasm_hip_factorization_verify: fact->L is NULL (echelonize with opts->L = 1)");
	const struct spasm_csr *U = fact->U, *L = fact->L;
	const int n = A->n, m = A->m, r = U->n;
	const i64 prime = A->field->p;
	if (U->field->p != prime || L->field->p != prime)
		die("spasm_hip_factorization_verify: A is mod %lld, U mod %lld, L mod %lld", (long long) prime, (long long) U->field->p,
		    (long long) L->field->p);
	if (L->n != n || L->m != r || U->m != m)
		die("spasm_hip_factorization_verify: A is %d x %d, L %d x %d, U %d x %d", n, m, L->n, L->m, r, U->m);
	if (count <= 0)
		return;
	std::vector<char> pivotal((size_t) n, 0);
	for (int j = 0; j < r; j++) {
		const int i = fact->p[j];
		if (i < 0 || i >= n)
			die("spasm_hip_factorization_verify: pivot %d sits on row %d of %d", j, i, n);
		pivotal[i] = 1;
	}
	std::vector<spasm_ZZp> X((size_t) count * n), T((size_t) count * m, 0), Y((size_t) count * r, 0), Z((size_t) count * m, 0);
	for (int s = 0; s < count; s++) {
		Prng g;
		g.seed(prime, seeds[s], 0);
		for (int i = 0; i < n; i++) {
			const spasm_ZZp foo = g.next_zp();
			X[(size_t) s * n + i] = pivotal[i] ? foo : 0;
		}
	}
	spasm_hip_xApy_batch(A, count, X.data(), T.data());
	spasm_hip_xApy_batch(L, count, X.data(), Y.data());
	spasm_hip_xApy_batch(U, count, Y.data(), Z.data());
	for (int s = 0; s < count; s++) {
		correct[s] = true;
		for (int j = 0; j < m; j++)
			if (Z[(size_t) s * m + j] != T[(size_t) s * m + j])
				correct[s] = false;
	}
}

bool spasm_hip_factorization_verify(const struct spasm_csr *A, const struct spasm_lu *fact, u64 seed)
{
	bool correct = false;
	spasm_hip_factorization_verify_batch(A, fact, 1, &seed, &correct);
	return correct;
}

// the reference's text format, byte for byte (spasm_certificate.c:221-240)
void spasm_hip_rank_certificate_save(const struct spasm_rank_certificate *proof, FILE *f)
{
	const int r = proof->r;
	fprintf(f, "%d\n", r);
	fprintf(f, "%" PRId64 "\n", proof->prime);
	for (int i = 0; i < 32; i++)
		fprintf(f, "%02x", proof->hash[i]);
	fprintf(f, "\n");
	for (int k = 0; k < r; k++)
		fprintf(f, "%d ", proof->i[k]);
	fprintf(f, "\n");
	for (int k = 0; k < r; k++)
		fprintf(f, "%d ", proof->j[k]);
	fprintf(f, "\n");
	for (int k = 0; k < r; k++)
		fprintf(f, "%d ", proof->x[k]);
	fprintf(f, "\n");
	for (int k = 0; k < r; k++)
		fprintf(f, "%d ", proof->y[k]);
	fprintf(f, "\n");
}

// spasm_certificate.c:242-270, with two deliberate differences: the second list is read into j (the reference reads it into i
// again, :258-259, and leaves j uninitialised), and a file that ends before 4 r values have been read is refused (false).
bool spasm_hip_rank_certificate_load(FILE *f, struct spasm_rank_certificate *proof)
{
	int r;
	proof->i = proof->j = nullptr;
	proof->x = proof->y = nullptr;
	proof->r = 0;
	if (1 != fscanf(f, "%d", &r) || r < 0)
		return false;
	proof->r = r;
	proof->i = (int *) xcalloc(r, sizeof(int));
	proof->j = (int *) xcalloc(r, sizeof(int));
	proof->x = (spasm_ZZp *) xcalloc(r, sizeof(spasm_ZZp));
	proof->y = (spasm_ZZp *) xcalloc(r, sizeof(spasm_ZZp));
	if (1 != fscanf(f, "%" SCNd64 "\n", &proof->prime))
		return false;
	char hash[65];
	if (nullptr == fgets(hash, 65, f))
		return false;
	for (int i = 0; i < 32; i++) {
		char byte[3] = {hash[2 * i], hash[2 * i + 1], 0};
		proof->hash[i] = (u8) strtoul(byte, nullptr, 16);
	}
	for (int *list : {proof->i, proof->j, (int *) proof->x, (int *) proof->y})
		for (int k = 0; k < r; k++)
			if (1 != fscanf(f, "%d", &list[k]))
				return false;
	return true;
}

// what spasm_hip_certificate_rank_create returns: its four lists and the struct
void spasm_hip_rank_certificate_free(struct spasm_rank_certificate *proof)
{
	if (proof == nullptr)
		return;
	free(proof->i);
	free(proof->j);
	free(proof->x);
	free(proof->y);
	free(proof);
}

}  // extern "C"
