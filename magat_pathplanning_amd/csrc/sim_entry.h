// The host side of the row-board kernels' entries: the refusal ladder they share and the launch of a wide kernel by its word count.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

#include "magat_common.h"

// The refusal ladder of an entry, in its order: a null pointer, a non-positive shape, a limit, the workspace's size, its alignment.
inline int sim_entry_check(std::initializer_list<const void*> pointers, bool shape_ok, bool limits_ok, const void* workspace,
                           size_t workspace_bytes, size_t need) {
  for (const void* p : pointers)
    if (!p) return MAGAT_ERR_NULL;
  if (!workspace) return MAGAT_ERR_NULL;
  if (!shape_ok) return MAGAT_ERR_BAD_SHAPE;
  if (!limits_ok || workspace_bytes < need) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(unsigned long long)) return MAGAT_ERR_WORKSPACE;
  return MAGAT_OK;
}
// launch(std::integral_constant<int, NW>) for the NW = 1, 2 or 4 words of a wide kernel's row (words: wide_words(W))
template <typename Launch>
inline void wide_launch(int words, Launch launch) {
  if (words == 1) launch(std::integral_constant<int, 1>{});
  else if (words == 2) launch(std::integral_constant<int, 2>{});
  else launch(std::integral_constant<int, 4>{});
}
