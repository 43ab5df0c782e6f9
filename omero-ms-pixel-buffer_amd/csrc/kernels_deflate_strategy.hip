// kernels_deflate_strategy.hip — k_lz77's HUFFMAN_ONLY and AUTO instantiations (deflate_seg.h
// STRAT_*, pbx_set_deflate_strategy) as a translation unit of their own: kernels_deflate.hip
// compiled down to k_lz77, what it calls and launch_lz77_strategy.  Kept apart so that the
// DEFAULT strategy's kernels in kernels_deflate.hip compile exactly as they did before the
// option existed (see the note above launch_lz77_strategy there).
#define PBX_LZ_STRATEGY_TU 1
#include "kernels_deflate.hip"
