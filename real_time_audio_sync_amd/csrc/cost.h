// Cell costs more than one kernel file uses (csrc/otw.hip, csrc/locate.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace rts {

// np.sqrt(np.sum((a-b)**2)) with numpy's pairwise order for 12 terms (oracle: orc_euclid).
__device__ __forceinline__ double euclid12(const double (&a)[12], const double (&b)[12]) {
    double sq[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const double d = a[i] - b[i];
        sq[i] = d * d;
    }
    double res = ((sq[0] + sq[1]) + (sq[2] + sq[3])) + ((sq[4] + sq[5]) + (sq[6] + sq[7]));
    res = res + sq[8];
    res = res + sq[9];
    res = res + sq[10];
    res = res + sq[11];
    return sqrt(res);
}

}  // namespace rts
