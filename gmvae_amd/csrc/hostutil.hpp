// What the host sides of the translation units (gmvae_hip.hip, tsne.hip, mixfit.hip, neigh.hip, ais.hip, linprobe.hip, twosample.hip) share: pointer
// alignment (a null pointer is aligned), the workspaces' 256-byte rounding, the once-per-device guard, and the evaluators' pointer
// ladder and LDS attribute.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/gmvae_hip.h"

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

// The pointer ladder of the model-independent evaluators (mixfit.hip, linprobe.hip), in the header's order -- NULL, then alignment:
// `required` may not be NULL; they and the `optional` outputs are 4-byte aligned, the workspace (required too) 16
typedef std::initializer_list<const void*> Pointers;
inline int check_pointers(Pointers required, Pointers optional, const void* workspace) {
  for (const void* p : required)
    if (!p) return GMVAE_E_NULL;
  if (!workspace) return GMVAE_E_NULL;
  for (const void* p : required)
    if (!aligned_to(p, 4)) return GMVAE_E_ALIGN;
  for (const void* p : optional)
    if (!aligned_to(p, 4)) return GMVAE_E_ALIGN;
  return aligned_to(workspace, 16) ? 0 : GMVAE_E_ALIGN;
}

// one-shot per DEVICE (`seen` is the caller's table): these kernels may ask for up to `bytes` of dynamic LDS, past the 64 KiB default
inline void allow_lds(bool (&seen)[64], Pointers kernels, int bytes) {
  if (!first_on_device(seen)) return;
  for (const void* k : kernels) hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace gmvae
