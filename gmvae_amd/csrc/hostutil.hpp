// What the host sides of the evaluators' translation units (tsne.hip, mixfit.hip, neigh.hip, ais.hip) share: pointer alignment
// (a null pointer is aligned) and the workspaces' 256-byte rounding.
#pragma once
#include <stdint.h>

namespace gmvae {

inline int aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline uint64_t up256(uint64_t b) { return (b + 255) / 256 * 256; }

}  // namespace gmvae
