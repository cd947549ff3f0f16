// What the host sides of the translation units (gmvae_hip.hip, tsne.hip, mixfit.hip, neigh.hip, ais.hip) share: pointer alignment
// (a null pointer is aligned), the workspaces' 256-byte rounding, and the once-per-device guard.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmvae {

inline int aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline uint64_t up256(uint64_t b) { return (b + 255) / 256 * 256; }

// one-shot per DEVICE (hipFuncSetAttribute belongs to the device's code object; a process may drive several devices): true the
// first time `seen`, the caller's static table, meets the current device -- and every time where the device cannot be told
inline bool first_on_device(bool (&seen)[64]) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return true;
  if (seen[dev]) return false;
  seen[dev] = true;
  return true;
}

}  // namespace gmvae
