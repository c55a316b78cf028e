// check_cert: verifies a rank certificate against a matrix (the reference's tools/check_cert.c, same options):
//     check_cert --matrix M.sms --modulus p --certificate FILE
// prints "CORRECT certificate" and exits 0 when it holds, "INCORRECT certificate" and exits 1 otherwise.  (The reference
// prints the two messages the wrong way round and returns 1 for a correct certificate, check_cert.c:75-80; not copied.)
// A wide matrix is transposed first, as tools/rank does before it factorizes (-t / --no-transpose: never), so that what rank
// certified -- the matrix it factorized, under the hash of the input file -- is what is checked.  The reference's check_cert
// never transposes.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>

#include "spasm_hip.h"

int main(int argc, char **argv)
{
	const char *filename = nullptr, *cert_file = nullptr;
	i64 prime = 42013;
	bool allow_transpose = true;
	static struct option longopts[] = {
		{"matrix", required_argument, nullptr, 'm'},
		{"modulus", required_argument, nullptr, 'p'},
		{"certificate", required_argument, nullptr, 'c'},
		{"no-transpose", no_argument, nullptr, 't'},
		{nullptr, 0, nullptr, 0}};
	int ch;
	while ((ch = getopt_long(argc, argv, "m:p:c:t", longopts, nullptr)) != -1) {
		switch (ch) {
		case 'm': filename = optarg; break;
		case 'p': prime = atoll(optarg); break;
		case 'c': cert_file = optarg; break;
		case 't': allow_transpose = false; break;
		default: fprintf(stderr, "unknown option\n"); return 2;
		}
	}
	if (cert_file == nullptr) {
		fprintf(stderr, "check_cert: --certificate FILE is required\n");
		return 2;
	}
	FILE *f = stdin;
	if (filename != nullptr) {
		f = fopen(filename, "r");
		if (f == nullptr) {
			perror(filename);
			return 2;
		}
	}
	u8 hash[32];
	struct spasm_triplet *T = spasm_hip_triplet_load(f, prime, hash);
	if (f != stdin)
		fclose(f);
	if (allow_transpose && T->n < T->m)
		spasm_hip_triplet_transpose(T);
	struct spasm_csr *A = spasm_hip_compress(T);
	spasm_hip_triplet_free(T);

	FILE *c = fopen(cert_file, "r");
	if (c == nullptr) {
		perror(cert_file);
		return 2;
	}
	struct spasm_rank_certificate proof;
	const bool loaded = spasm_hip_rank_certificate_load(c, &proof);
	fclose(c);
	const bool correct = loaded && spasm_hip_certificate_rank_verify(A, hash, &proof);
	fprintf(stderr, correct ? "CORRECT certificate\n" : "INCORRECT certificate\n");
	free(proof.i);
	free(proof.j);
	free(proof.x);
	free(proof.y);
	spasm_hip_csr_free(A);
	return correct ? 0 : 1;
}
