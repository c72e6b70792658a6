// Stand-alone driver of csrc/gru_tiles.h for tests/test_gru_tiles.py: built with -fsanitize=address,undefined, results on stdout.
//   gru_tiles_check <cus> <B>     prints one line "begin end MS" per range the rule yields for a batch of B on <cus> compute units
#include <cstdio>
#include <cstdlib>
#include "gru_tiles.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: gru_tiles_check <cus> <B>\n"); return 2; }
    return cto::for_each_gru_tile_range(atoll(argv[2]), atoi(argv[1]), [](int64_t begin, int64_t end, auto ms) {
        printf("%lld %lld %d\n", (long long)begin, (long long)end, int(decltype(ms)::value));
        return 0;
    });
}
