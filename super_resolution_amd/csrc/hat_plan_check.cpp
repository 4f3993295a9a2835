// hat_plan_check.cpp — would hat_plan_load take this file?  The host half of the loader (hat_plan_parse.h) behind a main():
// no HIP, no GPU, nothing to link but the C++ runtime, so it builds with any host compiler — and under its sanitizers, which
// is how tests/test_plan_parse_cpu.py runs it.  Not part of libhat_mi355x.so.
//
//     c++ -std=c++17 -Iinclude super_resolution_amd/csrc/hat_plan_check.cpp -o hat_plan_check
//     hat_plan_check net.hatplan ...      one line per file: "accept <path>" or "refuse <code> <path>"; exit 0 if all were accepted, else 1
//     hat_plan_check --manifest list.txt  the same for the paths in list.txt (one per line); always exit 0: the lines are the result
//     hat_plan_check --table              the signature table: "<id> <name> <nargs> <kind>[:<bytes>] ..." per function
#include <stdio.h>
#include <string.h>

#include <new>
#include <string>

#include "hat_plan_parse.h"

using namespace hat_plan_host;

static int check(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return HAT_EINVAL;
    int rc;
    try {
        Parsed parsed;
        rc = hat_plan_parse(f, &parsed);
    } catch (const std::bad_alloc&) {   // (what hat_plan_load's catch turns into HAT_EINVAL)
        rc = HAT_EINVAL;
    }
    fclose(f);
    return rc;
}

static bool report(const char* path) {
    const int rc = check(path);
    if (rc) printf("refuse %d %s\n", rc, path);
    else printf("accept %s\n", path);
    return rc == 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && strcmp(argv[1], "--table") == 0) {
        for (uint32_t i = 0; i < N_FN; ++i) {
            const Signature& s = SIGNATURES[i];
            printf("%u %s %u", i, s.name, s.nargs);
            for (uint32_t k = 0; k < s.nargs; ++k) {
                printf(" %s", kind_name(s.p[k].kind));
                if (s.p[k].bytes) printf(":%u", s.p[k].bytes);
            }
            printf("\n");
        }
        return 0;
    }
    if (argc == 3 && strcmp(argv[1], "--manifest") == 0) {
        FILE* m = fopen(argv[2], "r");
        if (!m) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
        char line[4096];
        while (fgets(line, sizeof(line), m)) {
            line[strcspn(line, "\r\n")] = 0;
            if (line[0]) report(line);
        }
        fclose(m);
        return 0;
    }
    if (argc < 2 || argv[1][0] == '-') {
        fprintf(stderr, "usage: %s <plan file> ... | --manifest <list> | --table\n", argv[0]);
        return 2;
    }
    bool all = true;
    for (int i = 1; i < argc; ++i) all = report(argv[i]) && all;
    return all ? 0 : 1;
}
