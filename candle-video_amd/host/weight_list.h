// Internal (host-only builds included): the ltx_weight list of an open safetensors file, for the *_create_from_file functions.
#pragma once
#include <functional>
#include <vector>
#include "../../include/ltxhip_weights.h"

// Appends to *out the tensors whose name `keep` accepts; name and data point into the mapping (alive until ltx_safetensors_close).
// A kept tensor that is not F32 / BF16, has more than 5 dimensions or a byte count that contradicts its shape fails, with `who` in
// front of the message; the others are never looked at.
int ltx_safetensors_weight_list(const ltx_safetensors* st, const char* who, const std::function<bool(const char*)>& keep, std::vector<ltx_weight>* out);
