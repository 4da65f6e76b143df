// kbench_io_echo.cpp -- puts the harnesses' file reader and writer (kbench_io.h) through a host compiler: reads a typed-array case file with
// read_launch and writes every array back with write_arrays, 64 entries of 0xA5 appended -- what a harness whose launch copied every input to an
// output would write.  No HIP, no GPU; tests/test_harness_io_cpu.py compiles it and feeds it well-formed and malformed files.
// usage: kbench_io_echo <case file> <result file> <magic in> <magic out> <multi 0|1> <max type> <max arrays> <max B> <max count>
// result: single { magic out, 0, 64, n_arrays } + arrays; multi { magic out, 64, n_launches } then per launch { op, n_arrays } + arrays
#include "kbench_io.h"
#include <cstdlib>

int main(int argc, char** argv) {
    if (argc < 10 || strlen(argv[3]) != 8 || strlen(argv[4]) != 8) { printf("usage: %s <case> <result> <magic in> <magic out> <multi> <max type> <max arrays> <max B> <max count>\n", argv[0]); return 2; }
    const bool multi = atoi(argv[5]) != 0;
    const CaseLimits lim{1 << 20, 1, atoll(argv[8]), atoll(argv[7]), atoll(argv[6]), atoll(argv[9])};
    const long long guard = 64;
    FILE* fi; long long nL = 1;
    if (const char* err = open_case(argv[1], argv[3], multi ? &nL : nullptr, &fi)) BAD(err);
    // everything is read before the result file is opened: a refused case leaves no result
    std::vector<Launch> launches((size_t)nL);
    for (Launch& L : launches) if (const char* err = read_launch(fi, lim, &L)) BAD(err);
    if (const char* err = close_case(fi)) BAD(err);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) BAD("cannot write the result file");
    bool ok = true;
    if (multi) { const long long oh[3] = {magic_word(argv[4]), guard, nL}; ok = write_arrays(fo, oh, 3, {}); }
    for (const Launch& L : launches) {
        std::vector<std::vector<char>> bytes;
        std::vector<HostArr> arrays;
        for (long long i = 0; i < L.nA; ++i) {
            bytes.push_back(L.A[i].bytes);
            bytes.back().resize(bytes.back().size() + (size_t)guard * tsize(L.A[i].type), (char)0xA5);
        }
        for (long long i = 0; i < L.nA; ++i) arrays.push_back({L.A[i].type, (size_t)(L.A[i].count + guard), bytes[i].data()});
        const long long single[4] = {magic_word(argv[4]), 0, guard, L.nA}, per[2] = {L.op, L.nA};
        ok = ok && (multi ? write_arrays(fo, per, 2, arrays) : write_arrays(fo, single, 4, arrays));
    }
    if (!ok || fclose(fo) != 0) BAD("write failed");
    printf("launches %lld\n", nL);
    return 0;
}
