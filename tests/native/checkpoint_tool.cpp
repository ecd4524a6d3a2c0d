// checkpoint_tool.cpp -- the host-only checkpoint reader and writer (mg-gcn_amd/host/checkpoint.hpp) as a stand-alone
// program for tests/test_checkpoint_cpu.py, built there by plain g++ under AddressSanitizer + UBSan:
//   checkpoint_tool <in> <out>   reads <in> and writes it back to <out>; prints "ok <tensors> <optimizer> <step>"
// A malformed file is exit status 3 and the reader's message on stderr.
#include <iostream>

#include "checkpoint.hpp"

int main(int argc, char **argv) {
    if (argc != 3) {
        std::cerr << "usage: checkpoint_tool <in> <out>" << std::endl;
        return 2;
    }
    try {
        const auto c = mggcn::checkpoint::read(argv[1]);
        c.write(argv[2]);
        std::cout << "ok " << c.tensors.size() << ' ' << (int)c.optimizer << ' ' << c.step << std::endl;
    } catch (const mggcn::checkpoint_error &e) {
        std::cerr << "checkpoint_error: " << e.what() << std::endl;
        return 3;
    }
    return 0;
}
