// LoRA adapter files (include/ltxhip_lora.h): the key parser and the safetensors loader.  Host-only C++ without HIP calls, so the
// host sanitizer build compiles it; the tensors themselves are uploaded by ltx_lora_create (csrc/lora.hip).
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ltxhip_lora.h"
#include "weight_list.h"
#include "../csrc/errors.h"

namespace {

bool starts_with(const std::string& s, const char* p) { const size_t n = strlen(p); return s.size() >= n && s.compare(0, n, p) == 0; }
bool ends_with(const std::string& s, const char* p) { const size_t n = strlen(p); return s.size() >= n && s.compare(s.size() - n, n, p) == 0; }

struct Suffix { const char* text; int role; };
const Suffix kSuffixes[] = {{".lora_A.weight", 0}, {".lora_B.weight", 1}, {".lora_down.weight", 0}, {".lora_up.weight", 1},
                            {".lora.down.weight", 0}, {".lora.up.weight", 1}, {".alpha", 2}};
// longest first: "model.diffusion_model." also ends in "diffusion_model."
const char* const kPrefixes[] = {"model.diffusion_model.", "diffusion_model.", "transformer."};

}  // namespace

extern "C" int ltx_lora_parse_key(const char* key, char* module_out, size_t cap, int* role) {
    if (!key || !module_out || !role) LTX_FAIL(LTX_ERR_ARG, "ltx_lora_parse_key: null argument");
    std::string k = key;
    int found = -1;
    for (const Suffix& s : kSuffixes)
        if (ends_with(k, s.text)) { found = s.role; k.resize(k.size() - strlen(s.text)); break; }
    if (found < 0) LTX_FAIL(LTX_ERR_ARG, std::string("ltx_lora_parse_key: '") + key + "' is not an adapter tensor name");
    for (const char* p : kPrefixes)
        if (starts_with(k, p)) { k.erase(0, strlen(p)); break; }
    if (k.empty()) LTX_FAIL(LTX_ERR_ARG, std::string("ltx_lora_parse_key: '") + key + "' names no module");
    std::vector<char> buf(k.size() + 64);      // (the remapper only ever shortens or slightly lengthens a name)
    LTX_TRY(ltx_weights_remap_key(k.c_str(), buf.data(), buf.size()));
    const size_t n = strlen(buf.data());
    if (n + 1 > cap) LTX_FAIL(LTX_ERR_ARG, "ltx_lora_parse_key: output buffer too small");
    memcpy(module_out, buf.data(), n + 1);
    *role = found;
    return LTX_OK;
}

#ifndef LTX_HOST_ONLY          /* the sanitizer build has no device library to create adapters in */
extern "C" int ltx_lora_create_from_file(const ltx_dit* like, const char* path, int strict, ltx_lora** out, int* n_unmatched) {
    if (n_unmatched) *n_unmatched = 0;
    if (!like || !path || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_lora_create_from_file: null argument");
    *out = nullptr;
    ltx_safetensors* st = nullptr;
    LTX_TRY(ltx_safetensors_open(path, &st));
    std::vector<ltx_weight> ws;      // not an adapter tensor: ignored, as ltx_lora_create does
    int rc = ltx_safetensors_weight_list(st, "ltx_lora_create_from_file", [](const char* name) {
        char mod[512]; int role = 0;
        return ltx_lora_parse_key(name, mod, sizeof(mod), &role) == LTX_OK; }, &ws);
    if (rc == LTX_OK) rc = ltx_lora_create(like, ws.data(), ws.size(), strict, out, n_unmatched);
    ltx_safetensors_close(st);
    return rc;
}
#endif
