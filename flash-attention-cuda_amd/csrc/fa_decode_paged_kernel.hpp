// Decode attention over a PAGED K/V cache for gfx950: the twin of
// fa_decode_kernel.hpp whose cache is a pool of fixed-size pages
//   k_pages, v_pages  [num_pages][Hkv][page_size][D]   (page_size % 64 == 0)
// plus a block table int32[B][max_pages]: entry j of row b is the pool page
// that holds keys [j * page_size, (j + 1) * page_size) of batch element b.
//
// It is the same kernel template (fa_decode_kernel<..., PAGED = true>): the
// same (batch, kv head, row group, piece) workgroups, wave w streams the same
// tiles t0 + w, t0 + w + 4, ... with the same operations in the same order,
// the same in-CU merge and the same in-launch piece merge through the
// workspace.  A 64-key tile never straddles a page, so all that differs per
// tile is the K and V buffer descriptor: its base is head hk's rows of the
// tile's page (64-bit arithmetic, pools exceed 4 GiB), its range ends at the
// tile's last live row, (tile % tiles_per_page) * 64 + clamp(len_b - 64 tile,
// 0, 64) rows, and the loads add the tile's offset in the page.  Rows past the
// length and unmapped pages are therefore never read, and a page id outside
// the pool gives a zero range.  Output and LSE are bit-identical to the
// contiguous kernel on the gathered cache with the same num_splits.
#pragma once

#include "fa_decode_kernel.hpp"

namespace fa {

// the twelve instantiations fa_decode_paged.hip launches
template <class T, int HDIM, int NB>
constexpr auto fa_decode_paged_kernel = fa_decode_kernel<T, HDIM, NB, true, DecodePagedParams>;

}  // namespace fa
