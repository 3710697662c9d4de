// batch_image.h -- the LDS images of the batch kernels (batch.hip: k_batch_admm_lds, k_batch_admm_reg): which form a batch runs and every byte those
// kernels read from LDS, planned in host-only steps (batch_image.cpp: no HIP header, integers and copies; one object per library).  The kernels take
// every array of a plan on trust; what they take for granted is checked on the CPU by tests/test_batch_image_host.py through
// tests/batch_image_probe.cpp.  DESIGN.md ("The LDS images of a batch") names the steps.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "host_csr.h"

// header of a problem's LDS image: byte offsets from the start of the image
//   Aval[nnzA] Pval[nnzP] f64 | rbA/rbAT/rbPT int4 tiles | Arp[m+1] Acol[nnzA] Trp[n+1] u16 | Tpr[nnzA] u32 (p | row << 16) | Prp[n+1] Pcol[nnzP] u16
//   | Aord[m] Tord[n] u16 (stored-sorted form of the register-CG variant only: the row / column index at every stored position; oAord = 0 otherwise)
// where A' entries are (position into Aval | row << 16): A' shares A's values
struct LdsHdr { int nnzA, nnzP, nbA, nbAT, nbPT, oAval, oPval, oArp, oAcol, oTrp, oTpr, oPrp, oPcol, oRbA, oRbAT, oRbPT, bytes, oAord, oTord; };
static_assert(sizeof(LdsHdr) == 19 * sizeof(int), "LdsHdr is 19 ints: the kernels read it from the first bytes of every image");

// a row or a column of A with this many entries is walked by a whole wave (the LONG instantiations of the register kernel)
#define LONG_ROW 64
// bytes in front of the SLICED image in LDS: xv (512), tv (2 x 512), block-sum slots (2 per wave of 512 threads)
#define SL_WS0 ((long long)sizeof(cosmo_hip_real) * (512 + 2 * 512 + 2 * (512 / 64)))
// the CSR-stream tile limits of brow_blocks (internal.h: COSMO_NNZ_PER_BLOCK nonzeros, 4 * COSMO_BS rows; batch.hip asserts the equality)
constexpr int kRowBlockNnz = 2048, kRowBlockRows = 4 * 256;

// row-block boundaries of the CSR-stream schedule: rb[t] .. rb[t + 1] are the rows of tile t
void brow_blocks(const std::vector<int>& rowptr, int nrows, std::vector<int>& rb);

// the COSMO_HIP_BATCH_* switches (batch.hip reads the environment once per set_params); the defaults are those of an empty environment
struct BatchImageOpts {
  bool lds = true;             // LDS: 0 = no image, the streaming kernel
  int bs = 512;                // BS: workgroup size of the LDS-image kernel (256, 512 or 1024)
  bool ext = false;            // EXT: 1 = the extended-cone instantiations on batches without such cones
  bool reg = true;             // REG: 0 = the iterates stay in global memory (LDS-image kernel)
  bool sliced = true;          // SLICED: 0 = no sliced image
  bool long_rows = true;       // LONG: 0 = no cooperative long-row passes
  bool ldscg = true;           // LDSCG: 0 = no register-CG form of the LDS-image kernel's reduced solve
  bool ldscg_sorted = true;    // LDSCG_SORTED: 0 = that form computes in index order
  bool store_sorted = true;    // STORE_SORTED: 0 = a sorted assignment reads an image stored in index order
  bool sorted = true;          // SORTED: 0 = every thread of the register kernel computes the rows it owns
  bool color = true;           // COLOR: 0 = positions of the gathered vectors are indices
};

struct BatchImageIn {
  int nprob = 0; long long n = 0, m = 0;
  const std::vector<HostCsr> *A = nullptr, *AT = nullptr, *PT = nullptr;            // per member: A, A', [P | A'] (split = start of the A' part)
  const std::vector<std::vector<int32_t>> *um_A = nullptr, *um_PT = nullptr;        // source of every entry of A and of [P | A'] in the caller's [P_nzval | A_nzval]
  int npsd = 0, nmid = 0, n3 = 0;              // PSD cones of dimension > 1, those of side 17 .. 64, exponential / power cones
  bool aa_on = false;
  long long max_lds = 0;                       // LDS bytes a workgroup can have
};

struct BatchImagePlan {
  bool fits = false;                           // false: some member does not fit an image (or LDS = 0): the streaming kernel, nothing below is used
  std::string error;                           // non-empty: the staged A and A' of a member disagree
  int bs = 0;                                  // workgroup size of the image kernels
  int reg_mode = 0;                            // 0: LdsOps kernel, 1: register-resident <512, 1, 2>, 2: <512, 2, 4>
  bool long_rows = false;                      // a row or a column of A with >= LONG_ROW entries in some problem
  bool force_ext = false;
  bool want_sliced = false;                    // every member has a sliced image (the device side may still decline it)
  bool p_all_diag = false;                     // P diagonal (or empty rows) in every problem
  bool rcg_form = false, rcg_sorted = false, rcg_stored = false;      // register-CG form of the LDS-image kernel: taken, sorted assignment, sorted storage
  std::vector<std::vector<unsigned char>> imgs, imgs2; long long stride = 0, stride2 = 0;     // row-major / sliced image per member, largest size
  std::vector<int> permA, permT;               // compute assignment: slot s of thread t works on row permA[(k * JM + s) * 512 + t] (-1: none)
  std::vector<int> posN, posM;                 // positions of the gathered LDS vectors
  std::vector<int> qposA;                      // per problem: position of row i of A in the image's (sorted) storage order
  // sliced image: first entry | length << 16 of every thread's rows / column; diagonal of P when P is diagonal in all problems
  std::vector<uint32_t> slA, slT; std::vector<cosmo_hip_real> pdiag; std::vector<unsigned char> pdiag_has;
  // source of every value slot of the row-major image, of the sliced image, of Pval and of the member's row of pdiag (-1: padding / no entry)
  std::vector<std::vector<int32_t>> um_imgA, um_imgA2, um_imgP, um_pd;
};

void plan_batch_images(const BatchImageIn& in, const BatchImageOpts& o, BatchImagePlan& pl);
