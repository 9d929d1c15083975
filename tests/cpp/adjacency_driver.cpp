// Drives the reference's own AdjacencyMatrix (src/AdjacencyMatrix.cpp, compiled by tests/test_submap_collection_cpu.py against the
// stand-in headers of tests/cpp/ref_shim) through a list of operations read from stdin, one per line:
//   E a b   addEdge(a, b)          M a   markAsLoopClosureSubmap(a)
//   D a     print getDistanceToNearestLoopClosureSubmap(a)      A a b   print isAdjacent(a, b)
// and prints one line per D / A / failed M: the number, or THROW when the reference throws (std::out_of_range from .at()).
#include <iostream>
#include <stdexcept>
#include <string>

#include "open3d_slam/AdjacencyMatrix.hpp"

int main() {
  o3d_slam::AdjacencyMatrix m;
  std::string op;
  long long a, b;
  while (std::cin >> op) {
    try {
      if (op == "E") {
        std::cin >> a >> b;
        m.addEdge(a, b);
      } else if (op == "M") {
        std::cin >> a;
        m.markAsLoopClosureSubmap(a);
      } else if (op == "D") {
        std::cin >> a;
        std::cout << m.getDistanceToNearestLoopClosureSubmap(a) << "\n";
      } else if (op == "A") {
        std::cin >> a >> b;
        std::cout << (m.isAdjacent(a, b) ? 1 : 0) << "\n";
      }
    } catch (const std::exception&) {
      std::cout << "THROW\n";
    }
  }
  return 0;
}
