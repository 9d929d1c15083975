"""AdjacencyMatrix (include/open3d_slam/AdjacencyMatrix.hpp, src/AdjacencyMatrix.cpp): which submaps touch, by submap id, and which
of them took part in a loop closure.  SubmapCollection adds an edge at every switch of the active submap and after every loop closure;
place recognition asks how far the last finished submap is from the nearest loop-closure submap.  Host bookkeeping: a few ints per
submap."""
from __future__ import annotations

import collections

INT_MAX = 2**31 - 1  # std::numeric_limits<int>::max()


class AdjacencyMatrix:
    def __init__(self):
        self.adjacency_: dict[int, set[int]] = {}
        self.isLoopClosureSubmap_: dict[int, bool] = {}

    def addEdge(self, id1: int, id2: int):
        """AdjacencyMatrix.cpp:16-21: both ends lose their loop-closure mark (the reference resets them, even when they had one)."""
        self.adjacency_.setdefault(id1, set()).add(id2)
        self.adjacency_.setdefault(id2, set()).add(id1)
        self.isLoopClosureSubmap_[id1] = False
        self.isLoopClosureSubmap_[id2] = False

    def getDistanceToNearestLoopClosureSubmap(self, id_: int) -> int:
        """AdjacencyMatrix.cpp:23-54: breadth-first from `id_` to the first marked submap, max(0, hops - 1).  INT_MAX while no submap
        has ever been in an edge.  When no marked submap is reachable the search ends at the last submap it dequeued and the hops to
        THAT one are returned (the reference's loop leaves `v` there).  Raises KeyError for an id that was never in an edge, as the
        reference's .at() throws."""
        if not self.isLoopClosureSubmap_:
            return INT_MAX
        toProcess = collections.deque([id_])
        visited = {id_}
        parents: dict[int, int] = {}
        v = id_
        while toProcess:
            v = toProcess.popleft()
            if self._at(self.isLoopClosureSubmap_, v):
                break
            for adj in sorted(self._at(self.adjacency_, v)):  # std::set: ascending
                if adj not in visited:
                    visited.add(adj)
                    toProcess.append(adj)
                    parents[adj] = v
        distance = 0
        while v != id_:
            v = parents[v]
            distance += 1
        return max(0, distance - 1)

    def markAsLoopClosureSubmap(self, id_: int):
        self._at(self.isLoopClosureSubmap_, id_)
        self.isLoopClosureSubmap_[id_] = True

    def isAdjacent(self, id1: int, id2: int) -> bool:
        if id1 == id2:
            return True
        return id2 in self.adjacency_.get(id1, ())

    def clear(self):
        """AdjacencyMatrix.cpp:82-84: the edges only; the loop-closure marks stay (as in the reference)."""
        self.adjacency_.clear()

    @staticmethod
    def _at(d: dict, key: int):
        if key not in d:
            raise KeyError(f"AdjacencyMatrix: submap id {key} was never in an edge")
        return d[key]
