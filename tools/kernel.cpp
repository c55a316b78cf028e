// kernel: drop-in for the reference's tools/kernel (tools/kernel.c + tools/common.c): same options, loads A (stdin or --matrix),
// transposes it first with --left, echelonizes it, and writes a basis of its right kernel, one vector per row, as an SMS matrix
// (--output FILE, else stdout); "Kernel basis matrix is n x m with nz nz" on stderr like the reference.  The basis is formed on
// the GPU (spasm_hip_kernel_basis).  One addition, --check: the rows of K, at most 64 dense rows at a time, are multiplied by
// A^T on the GPU (spasm_hip_transpose_device, spasm_hip_xApy_batch); "CORRECT kernel basis" and exit status 0 when every product
// is zero, "INCORRECT kernel basis" and 1 otherwise (checked before K is written: an incorrect basis leaves no output).
#include <getopt.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spasm_hip.h"

// K . A^T == 0, the rows of K in blocks of at most 64
static bool check(const struct spasm_csr *A, const struct spasm_csr *K)
{
	struct spasm_csr *At = spasm_hip_transpose_device(A, 1);
	const int m = A->m, n = A->n;
	bool ok = true;
	for (int k0 = 0; k0 < K->n && ok; k0 += 64) {
		const int k = std::min(64, K->n - k0);
		std::vector<spasm_ZZp> X((size_t) k * std::max(m, 1), 0), Y((size_t) k * std::max(n, 1), 0);
		for (int v = 0; v < k; v++)
			for (i64 px = K->p[k0 + v]; px < K->p[k0 + v + 1]; px++)
				X[(size_t) v * m + K->j[px]] = K->x[px];
		spasm_hip_xApy_batch(At, k, X.data(), Y.data());
		for (size_t t = 0; t < (size_t) k * n; t++)
			ok = ok && Y[t] == 0;
	}
	spasm_hip_csr_free(At);
	return ok;
}

int main(int argc, char **argv)
{
	struct echelonize_opts opts;
	spasm_hip_echelonize_init_opts(&opts);
	const char *filename = nullptr, *output_filename = nullptr;
	i64 prime = 42013;
	bool left = false, do_check = false;
	enum { NO_LOW_RANK = 1000, NO_DENSE, NO_GPLU, MAX_ITER, DENSE_THR, MIN_PIV, DENSE_BLK, MIN_RANK, MAX_ASPECT, NO_GREEDY, CHECK };
	static struct option longopts[] = {
		{"matrix", required_argument, nullptr, 'm'},
		{"modulus", required_argument, nullptr, 'p'},
		{"left", no_argument, nullptr, 'l'},
		{"output", required_argument, nullptr, 'o'},
		{"check", no_argument, nullptr, CHECK},
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
	while ((ch = getopt_long(argc, argv, "m:p:lo:", longopts, nullptr)) != -1) {
		switch (ch) {
		case 'm': filename = optarg; break;
		case 'p': prime = atoll(optarg); break;
		case 'l': left = true; break;
		case 'o': output_filename = optarg; break;
		case CHECK: do_check = true; break;
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
	FILE *in = stdin;
	if (filename != nullptr) {
		in = fopen(filename, "r");
		if (in == nullptr) {
			perror(filename);
			return 1;
		}
	}
	struct spasm_triplet *T = spasm_hip_triplet_load(in, prime, nullptr);
	if (in != stdin)
		fclose(in);
	if (left) {
		fprintf(stderr, "Left-kernel, transposing\n");
		spasm_hip_triplet_transpose(T);
	}
	struct spasm_csr *A = spasm_hip_compress(T);
	spasm_hip_triplet_free(T);
	struct spasm_lu *fact = spasm_hip_echelonize(A, &opts);
	struct spasm_csr *K = spasm_hip_kernel_basis(fact);
	fprintf(stderr, "Kernel basis matrix is %d x %d with %lld nz\n", K->n, K->m, (long long) spasm_hip_nnz(K));
	// --check comes before the output: an INCORRECT basis is never written
	if (do_check) {
		const bool ok = check(A, K);
		fprintf(stderr, "%s kernel basis\n", ok ? "CORRECT" : "INCORRECT");
		if (!ok)
			return 1;
	}
	FILE *f = stdout;
	if (output_filename != nullptr) {
		f = fopen(output_filename, "w");
		if (f == nullptr) {
			perror(output_filename);
			return 1;
		}
	}
	spasm_hip_csr_save(K, f);
	if (f != stdout)
		fclose(f);
	spasm_hip_csr_free(K);
	spasm_hip_lu_free(fact);
	spasm_hip_csr_free(A);
	return 0;
}
