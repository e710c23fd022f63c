// The proving-key relation check's host mirror (polymath_amd/host/key_check.hpp) over serialised keys: no GPU, no library link.
//   key_check_runner <curve> <form> [hex ...]      curve: bls12_381 | bn254, form: compressed | uncompressed
// Every argument after the form is the hex of one ProvingKey; with none, one key a line is read from stdin.  One line a key:
// "ok" or the text of the first failing relation, or "malformed: <why>".  The weights' seed is fixed: the keys are fixed before it.
#include <cstdio>
#include <iostream>
#include <string>

#include "../../polymath_amd/host/key_check.hpp"
using namespace pmhost;

static Bytes unhex(const std::string &s) {
    Bytes b;
    auto nib = [](char ch) { return ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10; };
    for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)(nib(s[i]) << 4 | nib(s[i + 1])));
    return b;
}

template <class C>
static int run_key(const std::string &hex, int form) {
    uint8_t seed[32];
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(0xA5 ^ (29 * i));
    try {
        const Bytes bytes = unhex(hex);
        const int rel = key_check_host<C>(key_check_parse<C>(bytes.data(), bytes.size(), form), seed);
        printf("%s\n", rel == KEY_REL_NONE ? "ok" : key_relation_text(rel).c_str());
        return rel == KEY_REL_NONE ? 0 : 1;
    } catch (const std::exception &e) {
        printf("malformed: %s\n", e.what());
        return 1;
    }
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: key_check_runner <curve> <form> [hex ...]\n"); return 2; }
    const std::string curve = argv[1], form_name = argv[2];
    const int form = form_name == "uncompressed" ? PM_WIRE_UNCOMPRESSED : PM_WIRE_COMPRESSED;
    std::vector<std::string> keys(argv + 3, argv + argc);
    if (keys.empty())
        for (std::string line; std::getline(std::cin, line);)
            if (!line.empty()) keys.push_back(line);
    int bad = 0;
    for (const std::string &hex : keys) bad += curve == "bn254" ? run_key<pm::BnCurve>(hex, form) : run_key<pm::BlsCurve>(hex, form);
    return bad ? 1 : 0;
}
