// solve: drop-in for the reference's tools/solve (tools/solve.c + tools/common.c): same options, loads A (stdin or --matrix)
// and the right-hand sides B (--rhs FILE, else stdin), echelonizes A with L, solves X.A = B and writes X as an SMS matrix
// (--output FILE, else stdout).  A row of B with no solution gets "WARNING: no solution for row i" on stderr, like the
// reference, and its row of X is what the reference writes for it.  Everything heavy runs on the GPU through libspasm_hip.so.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/time.h>

#include "spasm_hip.h"

static double now()
{
	struct timeval tv;
	gettimeofday(&tv, nullptr);
	return tv.tv_sec + 1e-6 * tv.tv_usec;
}

static struct spasm_csr *load(const char *filename, i64 prime)
{
	FILE *f = stdin;
	if (filename != nullptr) {
		f = fopen(filename, "r");
		if (f == nullptr) {
			perror(filename);
			exit(1);
		}
	}
	u8 hash[32];
	struct spasm_triplet *T = spasm_hip_triplet_load(f, prime, hash);
	if (f != stdin)
		fclose(f);
	struct spasm_csr *A = spasm_hip_compress(T);
	spasm_hip_triplet_free(T);
	return A;
}

int main(int argc, char **argv)
{
	struct echelonize_opts opts;
	spasm_hip_echelonize_init_opts(&opts);
	const char *filename = nullptr, *rhs_filename = nullptr, *output_filename = nullptr;
	i64 prime = 42013;
	enum { NO_LOW_RANK = 1000, NO_DENSE, NO_GPLU, MAX_ITER, DENSE_THR, MIN_PIV, DENSE_BLK, MIN_RANK, MAX_ASPECT, NO_GREEDY };
	static struct option longopts[] = {
		{"matrix", required_argument, nullptr, 'm'},
		{"modulus", required_argument, nullptr, 'p'},
		{"rhs", required_argument, nullptr, 'r'},
		{"output", required_argument, nullptr, 'o'},
		{"no-low-rank-mode", no_argument, nullptr, NO_LOW_RANK},
		{"no-dense-mode", no_argument, nullptr, NO_DENSE},
		{"no-GPLU", no_argument, nullptr, NO_GPLU},
		{"no-greedy-pivot-search", no_argument, nullptr, NO_GREEDY},
		{"max-iterations", required_argument, nullptr, MAX_ITER},
		{"dense-threshold", required_argument, nullptr, DENSE_THR},
		{"min-pivot-proportion", required_argument, nullptr, MIN_PIV},
		{"dense-block-size", required_argument, nullptr, DENSE_BLK},
		{"min-rank-ratio", required_argument, nullptr, MIN_RANK},
		{"max-aspect-ratio", required_argument, nullptr, MAX_ASPECT},
		{nullptr, 0, nullptr, 0}};
	int ch;
	while ((ch = getopt_long(argc, argv, "m:p:r:o:", longopts, nullptr)) != -1) {
		switch (ch) {
		case 'm': filename = optarg; break;
		case 'p': prime = atoll(optarg); break;
		case 'r': rhs_filename = optarg; break;
		case 'o': output_filename = optarg; break;
		case NO_LOW_RANK: opts.enable_tall_and_skinny = 0; break;
		case NO_DENSE: opts.enable_dense = 0; break;
		case NO_GPLU: opts.enable_GPLU = 0; break;
		case NO_GREEDY: opts.enable_greedy_pivot_search = 0; break;
		case MAX_ITER: opts.max_round = atoi(optarg); break;
		case DENSE_THR: opts.sparsity_threshold = atof(optarg); break;
		case MIN_PIV: opts.min_pivot_proportion = atof(optarg); break;
		case DENSE_BLK: opts.dense_block_size = atoi(optarg); break;
		case MIN_RANK: opts.low_rank_ratio = atof(optarg); break;
		case MAX_ASPECT: opts.tall_and_skinny_ratio = atof(optarg); break;
		default: fprintf(stderr, "unknown option\n"); return 1;
		}
	}
	if (optind < argc) {
		fprintf(stderr, "ERROR: invalid argument ``%s''\n", argv[optind]);
		return 1;
	}
	fprintf(stderr, "Loading A\n");
	struct spasm_csr *A = load(filename, prime);
	fprintf(stderr, "Loading B\n");
	struct spasm_csr *B = load(rhs_filename, prime);
	if (B->m != A->m) {
		fprintf(stderr, "ERROR: B has %d columns, A has %d\n", B->m, A->m);
		return 1;
	}
	fprintf(stderr, "Echelonizing A\n");
	fprintf(stderr, "start. A is %d x %d (%lld nnz)\n", A->n, A->m, (long long) A->p[A->n]);
	opts.L = 1;
	double t0 = now();
	struct spasm_lu *fact = spasm_hip_echelonize(A, &opts);
	fprintf(stderr, "echelonization done in %.3f s rank = %d\n", now() - t0, fact->U->n);
	fprintf(stderr, "Solving XA == B\n");
	bool *ok = (bool *) spasm_hip_malloc((i64) (B->n > 0 ? B->n : 1) * sizeof(bool));
	t0 = now();
	struct spasm_csr *X = spasm_hip_gesv(fact, B, ok);
	for (int i = 0; i < B->n; i++)
		if (!ok[i])
			fprintf(stderr, "WARNING: no solution for row %d\n", i);
	fprintf(stderr, "done in %.3f s\n", now() - t0);
	FILE *f = stdout;
	if (output_filename != nullptr) {
		f = fopen(output_filename, "w");
		if (f == nullptr) {
			perror(output_filename);
			return 1;
		}
	}
	spasm_hip_csr_save(X, f);
	if (f != stdout)
		fclose(f);
	free(ok);
	spasm_hip_csr_free(X);
	spasm_hip_lu_free(fact);
	spasm_hip_csr_free(B);
	spasm_hip_csr_free(A);
	return 0;
}
