// Host driver of the beam-search bookkeeping the kernel runs (tortoise_tts_amd/csrc/beam_book.h): a stand-alone CPU program, no GPU, no HIP.
//   c++ -O1 -std=c++17 [-fsanitize=address,undefined] tests/diag/beam_book_check.cpp -o beam_book_check
// stdin:  N max_new stop_token length_penalty, then per step the 2N picks as "flat_index log_prob" pairs (V follows N on the first line).
// stdout: per step one line: over | tok[N] | beam_idx[N] | running scores[N] | finished scores[N] | finished flags[N] | finished lengths[N] | heuristic bit |
//         the generated tokens of the running beams [N][steps so far] | those of the finished beams [N][max_new]
// tests/test_beam_ref.py feeds it the picks of the restated HF loop (tests/beam_ref.py) and compares every line with that loop's state.
#include <stdio.h>

#include <vector>

#include "../../tortoise_tts_amd/csrc/beam_book.h"

int main() {
	int N, V, max_new;
	long long stop;
	float length_penalty;
	if (scanf("%d %d %d %lld %f", &N, &V, &max_new, &stop, &length_penalty) != 5 || N < 1 || N > ttk::BEAM_MAX || max_new < 1) return 2;
	const int K = 2 * N;
	std::vector<float> scores(2 * N, -1e9f);
	scores[0] = 0.f;
	std::vector<int> state(2 * N + 1, 0);
	state[2 * N] = 1;
	std::vector<int64_t> tok(N), beam_idx(N);
	std::vector<long long> run((size_t)N * max_new, stop), fin((size_t)N * max_new, stop), nrun(run), nfin(fin);
	ttk::BeamBook book;
	for (int64_t c = 0; c < max_new; ++c) {
		for (int j = 0; j < K; ++j) {
			long long idx;
			float lp;
			if (scanf("%lld %f", &idx, &lp) != 2) return 0;      // end of input
			book.beam[j] = (int)(idx / V); book.tok[j] = idx % V; book.lp[j] = lp;
		}
		const int over = ttk::beam_bookkeep(book, N, c, max_new, stop, length_penalty, scores.data(), state.data(), tok.data(), beam_idx.data());
		for (int n = 0; n < N; ++n)
			for (int pos = 0; pos < max_new; ++pos) {      // the kernel's parallel copy into the other half of the sequence store
				nrun[(size_t)n * max_new + pos] = pos == c ? book.run_tok[n] : run[(size_t)book.run_src[n] * max_new + pos];
				const int fs = book.fin_src[n];
				nfin[(size_t)n * max_new + pos] = fs < 0 ? fin[(size_t)(-1 - fs) * max_new + pos] : (pos == c ? book.fin_tok[n] : run[(size_t)fs * max_new + pos]);
			}
		run = nrun; fin = nfin;
		printf("%d |", over);
		for (int n = 0; n < N; ++n) printf(" %lld", (long long)tok[n]);
		printf(" |");
		for (int n = 0; n < N; ++n) printf(" %lld", (long long)beam_idx[n]);
		printf(" |");
		for (int n = 0; n < N; ++n) printf(" %.9g", scores[n]);
		printf(" |");
		for (int n = 0; n < N; ++n) printf(" %.9g", scores[N + n]);
		printf(" |");
		for (int n = 0; n < N; ++n) printf(" %d", state[n]);
		printf(" |");
		for (int n = 0; n < N; ++n) printf(" %d", state[N + n]);
		printf(" | %d |", state[2 * N]);
		for (int n = 0; n < N; ++n)
			for (int pos = 0; pos <= c; ++pos) printf(" %lld", run[(size_t)n * max_new + pos]);
		printf(" |");
		for (int n = 0; n < N; ++n)
			for (int pos = 0; pos < max_new; ++pos) printf(" %lld", fin[(size_t)n * max_new + pos]);
		printf("\n");
		if (over) break;
	}
	return 0;
}
