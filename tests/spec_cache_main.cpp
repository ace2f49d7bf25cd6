// TEST INFRASTRUCTURE ONLY (tests/test_spec_cache.py): a stand-alone program around csrc/spec_cache.cpp, compiled with
// -fsanitize=address,undefined.  No GPU and no compiler: the objects it loads are stubs the test makes, HIPCC is a script.
//   spec_cache_main <a|b> op...     one line of output per op, in order
//   ops: find | find_verified | present | verified | build | forget | mark | reject | cp SRC DST | touch PATH | rm PATH
// find / find_verified print what the object's step entry returns ("none": nothing loaded); the stubs touch no argument.
#include <sys/stat.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "spec_cache.h"

using namespace mpcqp;

// a: the smallest line of spec_manifest.txt (3 2 7 12 4 1 cf), default blocking; b: nZ~ = 69 > 64, dense weights, two custom rows
static Dims dims(char which) {
    Dims d{};
    if (which == 'a') { d.nu = 3; d.ny = 2; d.nxh = 7; d.Hp = 12; d.Hc = 4; d.neps = 1; d.gmask = 0xcfu; }
    else { d.nu = 4; d.ny = 4; d.nxh = 8; d.Hp = 40; d.Hc = 17; d.neps = 1; d.gmask = 0xc8cu; d.dense_w = 1; d.nw = 2; }
    d.B = 1; d.default_nb = 1; d.nDU = d.nu * d.Hc; d.nZ = d.nDU + d.neps;
    return d;
}

static void show(const char* op, const SpecEntry& e, const Dims& d) {
    if (e.step) printf("%s %d\n", op, e.step(&d, nullptr, nullptr, nullptr));
    else printf("%s none\n", op);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const Dims d = dims(argv[1][0]);
    for (int i = 2; i < argc; ++i) {
        const std::string op = argv[i];
        if (op == "find") show("find", spec_find(d), d);
        else if (op == "find_verified") show("find_verified", spec_find_verified(d), d);
        else if (op == "present") printf("present %d\n", (int)spec_present(d));
        else if (op == "verified") printf("verified %d\n", (int)spec_verified(d));
        else if (op == "forget") { spec_forget_miss(d); printf("forget\n"); }
        else if (op == "mark") { mark_spec_verified(d); printf("mark\n"); }
        else if (op == "reject") { reject_spec(d); printf("reject\n"); }
        else if (op == "build") {
            std::string path, err;
            const int rc = spec_build(d, &path, &err);
            printf("build %d|%s|%s\n", rc, path.c_str(), err.c_str());
        } else if (op == "cp" && i + 2 < argc) {        // a NEW file (the loader knows a loaded object by its inode)
            (void)remove(argv[i + 2]);
            std::ofstream(argv[i + 2], std::ios::binary) << std::ifstream(argv[i + 1], std::ios::binary).rdbuf();
            chmod(argv[i + 2], 0644);
            printf("cp\n");
            i += 2;
        } else if (op == "touch" && i + 1 < argc) {
            std::ofstream(argv[++i]).flush();
            printf("touch\n");
        } else if (op == "rm" && i + 1 < argc) {
            printf("rm %d\n", remove(argv[++i]));
        } else {
            printf("unknown op %s\n", op.c_str());
            return 2;
        }
        fflush(stdout);
    }
    return 0;
}
