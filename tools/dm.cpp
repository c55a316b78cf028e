// dm: the Dulmage-Mendelsohn decomposition of a matrix (the reference's tools/dm.c, same options).  The matrix comes on stdin
// (SMS or MatrixMarket), modulo 42013.
//     --permuted   (default) prints A(p, q) in SMS
//     --verbose    the structural rank, H, S with the sizes of its strongly connected components, V
//     --tabulated  prints nothing (as the reference)
//     --image N    PNM output is not supported: exits 2
// The matching and the coarse decomposition run on the GPU (libspasm_hip.so); the blocks of S are found on the host.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>

#include "spasm_hip.h"

int main(int argc, char **argv)
{
	static struct option longopts[] = {
		{"permuted", no_argument, nullptr, 'p'},
		{"verbose", no_argument, nullptr, 'v'},
		{"tabulated", no_argument, nullptr, 't'},
		{"image", required_argument, nullptr, 'i'},
		{nullptr, 0, nullptr, 0}};
	char mode = 'p';
	int ch;
	while ((ch = getopt_long(argc, argv, "", longopts, nullptr)) != -1) {
		switch (ch) {
		case 'i':
			fprintf(stderr, "dm: PNM output is not supported\n");
			return 2;
		case 'p':
		case 'v':
		case 't':
			mode = (char) ch;
			break;
		default:
			fprintf(stderr, "dm: unknown option\n");
			return 1;
		}
	}
	struct spasm_triplet *T = spasm_hip_triplet_load(stdin, 42013, nullptr);
	struct spasm_csr *A = spasm_hip_compress(T);
	spasm_hip_triplet_free(T);
	const int m = A->m;
	struct spasm_dm *DM = spasm_hip_dulmage_mendelsohn(A);
	const int *rr = DM->rr, *cc = DM->cc;

	switch (mode) {
	case 't':
		break;
	case 'v': {
		printf("structural rank = %d\n", rr[2] + cc[4] - cc[3]);
		const int h_n = rr[1] - rr[0], h_m = cc[2] - cc[0];
		if (h_n > 0 && h_m > 0)
			printf("*) H (%d x %d)\n", h_n, h_m);
		const int s_n = rr[2] - rr[1], s_m = cc[3] - cc[2];
		if (s_n > 0 && s_m > 0) {
			printf("*) S (%d x %d) : \n", s_n, s_m);
			int n_trivial = 0;
			for (int b = 1; b < DM->nb - 1; b++) {
				const int size = DM->r[b + 1] - DM->r[b];
				if (size == 1)
					n_trivial++;
				else
					printf("    *) SCC of size %d\n", size);
			}
			if (n_trivial > 0)
				printf("    -> plus %d SCC of size 1\n", n_trivial);
		}
		const int v_n = rr[4] - rr[2], v_m = cc[4] - cc[3];
		if (v_n > 0 && v_m > 0)
			printf("*) V (%d x %d)\n", v_n, v_m);
		break;
	}
	case 'p': {
		int *qinv = spasm_hip_pinv(DM->q, m);
		struct spasm_csr *B = spasm_hip_permute(A, DM->p, qinv, 1);
		free(qinv);
		spasm_hip_csr_save(B, stdout);
		spasm_hip_csr_free(B);
		break;
	}
	}
	spasm_hip_dm_free(DM);
	spasm_hip_csr_free(A);
	return 0;
}
