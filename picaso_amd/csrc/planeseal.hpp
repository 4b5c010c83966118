// Seals of resident reflected plane sets (planeseal.hip): what the memory plumbing and the reflected launcher of
// api.hip need from the registry.  Not part of the C ABI.
#pragma once
#include <cstddef>

namespace pz {

// true when the eleven addresses (REFLECTED_PLANES order) with these sizes carry a seal whose flags are all set;
// layer_mask (two words) / mask_valid (both may be null): bit i set = layer i of that set is cloud-free in every column;
// not valid and all 0 when the seal recorded no mask (more than 128 layers) or there is no seal.
// deck_mask (two words) / w0_unit, handed out with a valid mask only: bit i set = layer i is cloudy and delta-scaled in every
// column (!(ftau_cld == 0) and !(dtau_og == dtau)); every w0 of the set lies in [0, 1]
bool seal_derivable(int device, const double *const planes[11], int nlevel, int nwno, long pitch,
                    unsigned long long *layer_mask = nullptr, bool *mask_valid = nullptr,
                    unsigned long long *deck_mask = nullptr, bool *w0_unit = nullptr);
// a launch took the LEVELS variant because of a seal (with_layer_mask: the LAYERS variant, which is counted as both)
void seal_count_hit(int device, bool with_layer_mask = false);
// drop every seal of the device with a plane that overlaps [p, p + bytes): the bytes are about to change or to go away
void seal_invalidate(int device, const void *p, size_t bytes);
// drop every seal of the device
void seal_drop_device(int device);

}  // namespace pz
