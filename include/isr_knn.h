/*
 * isr_knn.h — C ABI of the exact k-nearest-neighbour search of libisr_hip.so and of the local frames (normals) built on it.
 * generateCors.py:205-212 reduces the marching-cubes vertices to 1 000 points and calls
 * pytorch3d.ops.estimate_pointcloud_normals(fv, neighborhood_size=400); these entries are what that call needs.
 * The conventions are those of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work
 * enqueued on `stream`, no call synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.
 *
 * THE SEARCH.  With, in f32 (the chain of isr_radius.h),
 *     dx = t.x-q.x; dy = t.y-q.y; dz = t.z-q.z;  d2 = fmaf(dz, dz, fmaf(dy, dy, dx*dx))
 * row i of idx holds the K targets that are smallest under the order (d2, index), ascending: among equal distances the
 * lowest index comes first, at the cut as well as inside the list.  d2 orders as its unsigned bits (it is never negative).
 * qry and tgt may be the same array: a point then finds itself at d2 = 0.  Integers and bits, a function of the points and K
 * only — of no launch shape, and a query's row of no other query — and the same from the device entry and the _host entry
 * (csrc/knn.hpp states the rule once).
 * PRECONDITION: finite coordinates.  Non-finite ones never make an access leave the arrays and every written index lies in
 * [0, Nt); which indices is unspecified (a NaN d2 orders as the bits 0x7fc00000).
 *
 * THE FRAMES.  Per point i, all in f64, from the K neighbours j = idx[i, 0 .. K-1] in that order (an entry outside
 * [0, N) is clamped into it, so no access leaves pts):
 *     mean = (sum_j p_j) / K                                    (plain additions in row order, one division per axis)
 *     C    = (sum_j (p_j - mean)(p_j - mean)^T) / K             (six sums, each c = fma(d_a, d_b, c) in row order)
 * which is pytorch3d's get_point_covariances AS FAR AS IT IS KNOWN FROM MEMORY (unpinned: pytorch3d is not available).
 * C = V diag(l) V^T by cyclic Jacobi: at most 30 sweeps over (0,1), (0,2), (1,2), stopping before a sweep once
 * sum_{p<q} c_pq^2 <= 1e-30 sum_i c_ii^2; the rotation is the one of csrc/epnp.hpp.  Eigenvalues ascending (a tie keeps the
 * lower axis first) -> curvatures[i, 0..2]; frames[i, r, c] = component r of eigenvector c: column 0 is the normal.
 * With disambiguate != 0 (pytorch3d's _disambiguate_vector_directions, from memory): for columns 0 and 2,
 *     count = #{ j : fma(v_z, dz, fma(v_y, dy, v_x dx)) > 0 },  d = p_j - p_i;    the column is negated when 2 count < K;
 * then column 1 = cross(column 2, column 0): the frame is right-handed.  Without it the columns are Jacobi's, whatever
 * their signs and handedness.
 * All neighbours identical (C = 0): no rotation happens, the frame is the identity and the curvatures are 0; with
 * disambiguate both counts are 0, so the frame is diag(-1, 1, -1).  Never NaN for finite points.
 * A DIFFERENCE FROM pytorch3d: it subtracts the whole cloud's mean first, "for stability", and works in f32.  Here the
 * covariance is formed in f64 about the neighbourhood's own mean, so nothing depends on where the cloud lies.
 */
#ifndef ISR_KNN_H
#define ISR_KNN_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch isr_knn needs; 0 (and isr_last_error()) for a shape isr_knn refuses.  The brute-force plan keeps its
 * state in LDS: the figure is small and constant today and may grow with a later plan. */
size_t isr_knn_workspace_bytes(int Nq, int Nt, int K);

/* qry (Nq, 3), tgt (Nt, 3) f32 on the device -> idx (Nq, K) int32 and, unless null, d2 (Nq, K) f32.
 * Refused: K < 1, K > Nt, K > 1024, Nq < 1, Nt < 1, Nt > 2^24, null pointers (d2 excepted),
 * ws_bytes < isr_knn_workspace_bytes(Nq, Nt, K).  The workspace needs no preparation and may be reused. */
int isr_knn(const float* qry, int Nq, const float* tgt, int Nt, int K, int32_t* idx, float* d2, void* ws, size_t ws_bytes,
            isr_stream_t stream);

/* The same search as host code over HOST pointers: the tests' reference. */
int isr_knn_host(const float* qry, int Nq, const float* tgt, int Nt, int K, int32_t* idx, float* d2);

/* pts (N, 3) f32, idx (N, K) int32 (isr_knn(pts, pts)) on the device -> curvatures (N, 3), frames (N, 3, 3) f64.
 * Refused: N < 1, K < 1, K > 1024, null pointers. */
int isr_local_frames(const float* pts, int N, const int32_t* idx, int K, int disambiguate, double* curvatures, double* frames,
                     isr_stream_t stream);

/* The same frames as host code over HOST pointers: the tests' reference. */
int isr_local_frames_host(const float* pts, int N, const int32_t* idx, int K, int disambiguate, double* curvatures,
                          double* frames);

#ifdef __cplusplus
}
#endif

#endif /* ISR_KNN_H */
