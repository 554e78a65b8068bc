// Stand-in of this repository for Thrust's header of the same name (TEST INFRASTRUCTURE). thrust::partition promises no order
// inside the two groups; this one is std::stable_partition, the order the oracle's compaction keeps too.
#pragma once
#include <algorithm>
#include <vector>
#include "device_vector.h"
// every call appends {elements partitioned, elements for which pred holds}: the driver reads the per-bounce ray counts from it
inline std::vector<long> ref_partition_log;
namespace thrust {
template <class T, class Pred>
inline device_ptr<T> partition(device_ptr<T> first, device_ptr<T> last, Pred pred) {
    T* mid = std::stable_partition(first.p, last.p, pred);
    ref_partition_log.push_back((long)(last.p - first.p));
    ref_partition_log.push_back((long)(mid - first.p));
    return device_ptr<T>(mid);
}
}  // namespace thrust
