// Host sanitizer driver of the LoRA key parser (include/ltxhip_lora.h; host/lora.cpp built with ASan + UBSan, LTX_HOST_ONLY):
// every prefix x suffix spelling, Official-layout names, refusals, exact-fit and too-small output buffers, long and odd keys.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ltxhip_lora.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    const char* prefixes[] = {"", "transformer.", "diffusion_model.", "model.diffusion_model."};
    const struct { const char* s; int role; } suffixes[] = {{".lora_A.weight", 0}, {".lora_B.weight", 1}, {".lora_down.weight", 0}, {".lora_up.weight", 1},
                                                           {".lora.down.weight", 0}, {".lora.up.weight", 1}, {".alpha", 2}};
    const std::string mod = "transformer_blocks.12.attn2.to_out.0";
    for (const char* p : prefixes)
        for (const auto& s : suffixes) {
            const std::string key = std::string(p) + mod + s.s;
            std::vector<char> exact(mod.size() + 1);             // exactly large enough: a write past it is the sanitizer's to see
            int role = -1;
            CHECK(ltx_lora_parse_key(key.c_str(), exact.data(), exact.size(), &role) == 0);
            CHECK(role == s.role && mod == exact.data());
            std::vector<char> small(mod.size());                 // one byte short
            CHECK(ltx_lora_parse_key(key.c_str(), small.data(), small.size(), &role) != 0);
            CHECK(ltx_lora_parse_key(key.c_str(), small.data(), 0, &role) != 0);
        }
    char buf[256]; int role = 9;
    CHECK(ltx_lora_parse_key("model.diffusion_model.patchify_proj.lora_A.weight", buf, sizeof buf, &role) == 0 && !strcmp(buf, "proj_in") && role == 0);
    CHECK(ltx_lora_parse_key("transformer_blocks.3.attn1.q_norm.alpha", buf, sizeof buf, &role) == 0 && !strcmp(buf, "transformer_blocks.3.attn1.norm_q") && role == 2);
    const char* refused[] = {"", ".", ".alpha", "alpha", "transformer..alpha", "a.weight", "a.lora_A", "a.lora_A.weight.", "lora_A.weight", ".lora_A.weight"};
    for (const char* k : refused) { role = 9; CHECK(ltx_lora_parse_key(k, buf, sizeof buf, &role) != 0 && role == 9); }
    CHECK(ltx_lora_parse_key(nullptr, buf, sizeof buf, &role) != 0);
    CHECK(ltx_lora_parse_key("a.alpha", nullptr, 8, &role) != 0);
    CHECK(ltx_lora_parse_key("a.alpha", buf, sizeof buf, nullptr) != 0);
    // long keys, with and without a suffix; names the remapper lengthens ("encoder.down_blocks.N" tables)
    const std::string longmod(70000, 'x');
    std::vector<char> big(longmod.size() + 64);
    CHECK(ltx_lora_parse_key((longmod + ".lora_up.weight").c_str(), big.data(), big.size(), &role) == 0 && longmod == big.data() && role == 1);
    CHECK(ltx_lora_parse_key(longmod.c_str(), big.data(), big.size(), &role) != 0);
    std::string many;
    for (int i = 0; i < 200; ++i) many += "decoder.up_blocks.1.";
    CHECK(ltx_lora_parse_key((many + "alpha").c_str(), big.data(), 16, &role) != 0);                      // lengthened name, tiny buffer
    std::vector<char> huge(many.size() * 3 + 64);
    const int rc = ltx_lora_parse_key((many + "x.alpha").c_str(), huge.data(), huge.size(), &role);
    CHECK(rc == 0 || strstr(ltx_last_error(), "too small") != nullptr);                                  // either fits or is refused, never overrun
    if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
    printf("lora host sanitizer driver: clean\n");
    return 0;
}
