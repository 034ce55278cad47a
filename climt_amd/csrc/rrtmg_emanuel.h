// rrtmg_emanuel.h -- climt's EmanuelConvection (emanuel/component.py around convect43c.f90; the rule as the reference's own numpy
// statement emanuel/pure_python.py::_convect and _tlift gives it) for ONE column (rrtmg_hip_emanuel_convection).  Level 0 is the
// surface.  The reference component's configuration only: IPBL = 0 (its dry-adjustment block is not here), NTRA = 0 (no tracers),
// NL = nlay - 3 (the highest level convection may reach), MINORIG from the caller.
//
//   thermodynamics   GZ, CPN, H, LV, HM, TV of the levels 0 .. NL;  IHMIN: the level of minimum moist static energy at or above
//                    MINORIG - 1, capped at NL - 1;  NK: the level of maximum HM in MINORIG - 1 .. IHMIN -- the parcel's origin
//   exit, IFLAG 0    T[NK] < 250, Q[NK] <= 0 or IHMIN == NL - 1: no unstable origin; CBMF = 0
//   LCL              RH = Q[NK] / QS[NK], CHI = T[NK] / (1669 - 122 RH - T[NK]), PLCL = P[NK] pow(RH, CHI)
//   exit, IFLAG 2    PLCL < 200 or >= 2000 hPa; CBMF = 0
//   cloud base       ICB: the first level above NK with P < PLCL, at most NL - 1
//   exit, IFLAG 3    ICB >= NL - 1: cloud base at the top; CBMF = 0
//   lifting          emanuel_tlift, first to ICB (KK 1): dry adiabat below, two Newton steps on saturation at ICB -- with the reference's
//                    saturation formulae: Bolton's above 0 C, exp(23.33086 - 6111.72784 / T + 0.15215 log T) below
//   exit, IFLAG 0    CBMF == 0 and TVP[ICB] <= TV[ICB] - DTMAX: the parcel is too cold and nothing is convecting; CBMF UNTOUCHED
//   IFLAG 1          lifting to NL (KK 2); precipitation efficiency EP; the level of neutral buoyancy INB (and INB1), CAPE, FRAC;
//                    HP; the sub-cloud quasi-equilibrium: CBMF = max((1 - DAMP dt / DELT0) CBMF + 0.1 ALPHA DTMA, 0)
//   exit, IFLAG 1    CBMF == 0 and its old value == 0: convecting by flag, all tendencies zero
//   mixing           M[ICB+1 .. INB]; for every origin i and destination j in ICB .. INB the mixing fraction SIJ -- denominators of
//                    magnitude below 0.01 are SET TO 0.01, as the reference does -- and where 0 < SIJ < 0.9 QENT, UENT, VENT, ELIJ,
//                    MENT;  then MENT normalised over the spectrum of every i (ASIJ, SCRIT), the undiluted fallback where NENT == 0
//   downdraft        where EP[INB] >= 1e-4: i = INB .. 0, WDTRAIN, the rain / snow constants by T[i] > 273, REVAP by sqrt, EVAP,
//                    WATER, MP, QP, UP, VP;  PRECIP
//   tendencies       FT, FQ, FU, FV of the levels 0 .. INB;  IFLAG 4 where 2 g DPINV AMP1 >= 1 / dt (CFL);  the FRAC adjustment of
//                    INB and INB - 1;  the dp-weighted means of cpn FT + lv FQ, FU and FV subtracted; FU, FV scaled by 1 - CU
// Every operation is rounded on its own (contraction off), in the reference's order, Python's `sum` as the running sum from 0 that
// it is, `max(a, b)` and `min(a, b)` as Python's (the first argument unless the second is strictly larger / smaller).
//
// Storage: nlay has no upper bound, so a thread keeps NO array of its own; every loop is a for bounded by nlay.
//   1-D   kEmanuelSlabs1 work slabs [nlay+1][ccol], columns fastest (GZ .. QS below).  The reference allocates ND + 1 = nlay + 1
//         and reads at most index NL + 1 = nlay - 2: PH[i+2] (i <= NL - 1), M[INB+1], MP[i+1], WATER[i+1], WT[i+1], QP[i+1], T[i+1]
//         (i <= INB <= NL).  Of the inputs, pint has nlay + 1 rows and the others nlay: NL + 1 < nlay.
//   2-D   six slabs MENT, QENT, ELIJ, SIJ, UENT, VENT cut to the block that can ever be written: rows (origins) i = 2 .. NL, columns
//         (destinations) j = 1 .. NL, i.e. [nlay-4][nlay-3][ccol] -- ICB >= NK + 1 >= 1, the rows written are ICB + 1 .. INB and
//         the columns ICB .. INB, INB <= NL.  Of that block a column initialises and uses its own rows ICB+1 .. INB and columns
//         ICB .. INB; everything the reference reads outside it it never wrote: MENT, ELIJ and SIJ are 0 there and QENT[i][j] is Q[j],
//         so such a term is 0 * (...) = 0 or a 0 in a sum, and is left out -- SIJ[i][ICB-1] and SIJ[i][INB+1] are read as the 0 they
//         are.  (Leaving out an exact zero keeps every value; the sign of a zero sum is the one thing it can change.)
//   Bytes of work space per column: 8 (kEmanuelSlabs1 (nlay + 1) + 6 (nlay - 4) (nlay - 3)): 169 600 at 61 layers.
//   The tendencies are accumulated in the output arrays, which therefore may not be inputs.
// Index bounds: nlay >= 4 is required (NL >= 1: the cap NL - 1 of IHMIN is a level); convection needs 1 <= ICB <= NL - 2, so with
// fewer than 6 layers every column leaves by one of the first exits and the 2-D block, empty below 5 layers, is never touched.
//
// Pressures: pmid and pint are read as p * pressure_scale (hPa per resident unit; 1.0 is exact): the 1000 hPa of the LCL formula,
// the 200 / 2000 hPa limits and the downdraft constants make the rule not unit-free.  qs == nullptr: QS[i] is the reference's
// bolton_q_sat(T, 100 P, rd, rv) (_core/util.py).
//
// Plain C++: tools/emanuel_check.cpp runs every "thread" of a launch on the CPU; the kernel is in rrtmg_emanuel.hip.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_EMANUEL_HD __host__ __device__ inline
#else
#define RRTMG_EMANUEL_HD inline
#endif

namespace rrtmg {

enum EmanuelSlab1 { kEmGZ, kEmCPN, kEmH, kEmLV, kEmHM, kEmTV, kEmTVP, kEmTP, kEmCLW, kEmEP, kEmHP, kEmWATER, kEmEVAP, kEmWT, kEmMP, kEmM,
                    kEmLVCP, kEmQP, kEmUP, kEmVP, kEmQS, kEmNENT, kEmanuelSlabs1 };
enum EmanuelSlab2 { kEmMENT, kEmQENT, kEmELIJ, kEmSIJ, kEmUENT, kEmVENT, kEmanuelSlabs2 };

// doubles of work space per column
RRTMG_EMANUEL_HD size_t emanuel_work1(int nlay) { return (size_t)kEmanuelSlabs1 * (size_t)(nlay + 1); }
RRTMG_EMANUEL_HD size_t emanuel_work2(int nlay) { return nlay > 4 ? (size_t)kEmanuelSlabs2 * (size_t)(nlay - 4) * (size_t)(nlay - 3) : 0; }

struct EmanuelCall {
  int32_t ncol, nlay, minorig;
  int32_t ccol;                         // columns of the chunk: the stride of the work slabs
  int64_t col0;                         // first column of the chunk
  const double *t, *q, *u, *v, *pmid;   // [nlay][ncol]
  const double *pint;                   // [nlay+1][ncol]
  const double *cbmf;                   // [ncol]
  const double *qs;                     // [nlay][ncol] or nullptr
  double dt, pressure_scale;
  double elcrit, tlcrit, entp, sigd, sigs, omtrain, omtsnow, coeffr, coeffs, cu, beta, dtmax, alpha, damp, delt0;
  double cpd, cpv, cl, rv, rd, lv0, g, rowl;
  double *ft, *fq, *fu, *fv;            // [nlay][ncol]
  double *precip, *wd, *tprime, *qprime, *cape;   // [ncol] or nullptr
  int32_t *iflag;                       // [ncol] or nullptr
  double *ft_per_day;                   // [nlay][ncol] or nullptr
  double *cbmf_out;                     // [ncol]; may be cbmf
  double *w1, *w2;                      // work: emanuel_work1(nlay) and emanuel_work2(nlay) doubles per column of the chunk
};

struct EmanuelScalars { double precip, wd, tprime, qprime, cbmf, cape; int32_t iflag; };

RRTMG_EMANUEL_HD double emanuel_max(double a, double b) { return b > a ? b : a; }      // Python's max(a, b)
RRTMG_EMANUEL_HD double emanuel_min(double a, double b) { return b < a ? b : a; }      // Python's min(a, b)

#define EM_T(i) a.t[(size_t)(i) * N + col]
#define EM_Q(i) a.q[(size_t)(i) * N + col]
#define EM_U(i) a.u[(size_t)(i) * N + col]
#define EM_V(i) a.v[(size_t)(i) * N + col]
#define EM_P(i) (a.pmid[(size_t)(i) * N + col] * sc)
#define EM_PH(i) (a.pint[(size_t)(i) * N + col] * sc)
#define EM_FT(i) a.ft[(size_t)(i) * N + col]
#define EM_FQ(i) a.fq[(size_t)(i) * N + col]
#define EM_FU(i) a.fu[(size_t)(i) * N + col]
#define EM_FV(i) a.fv[(size_t)(i) * N + col]
#define EM_1(k, i) a.w1[((size_t)(k) * (size_t)(a.nlay + 1) + (size_t)(i)) * CC + lc]
#define EM_2(k, i, j) a.w2[(((size_t)(k) * (size_t)(a.nlay - 4) + (size_t)((i) - 2)) * (size_t)(a.nlay - 3) + (size_t)((j) - 1)) * CC + lc]
#define GZ(i) EM_1(kEmGZ, i)
#define CPN(i) EM_1(kEmCPN, i)
#define H(i) EM_1(kEmH, i)
#define LV(i) EM_1(kEmLV, i)
#define HM(i) EM_1(kEmHM, i)
#define TV(i) EM_1(kEmTV, i)
#define TVP(i) EM_1(kEmTVP, i)
#define TP(i) EM_1(kEmTP, i)
#define CLW(i) EM_1(kEmCLW, i)
#define EP(i) EM_1(kEmEP, i)
#define HP(i) EM_1(kEmHP, i)
#define WATER(i) EM_1(kEmWATER, i)
#define EVAP(i) EM_1(kEmEVAP, i)
#define WT(i) EM_1(kEmWT, i)
#define MP(i) EM_1(kEmMP, i)
#define M(i) EM_1(kEmM, i)
#define LVCP(i) EM_1(kEmLVCP, i)
#define QP(i) EM_1(kEmQP, i)
#define UP(i) EM_1(kEmUP, i)
#define VP(i) EM_1(kEmVP, i)
#define QS(i) EM_1(kEmQS, i)
#define NENT(i) EM_1(kEmNENT, i)
#define MENT(i, j) EM_2(kEmMENT, i, j)
#define QENT(i, j) EM_2(kEmQENT, i, j)
#define ELIJ(i, j) EM_2(kEmELIJ, i, j)
#define SIJ(i, j) EM_2(kEmSIJ, i, j)
#define UENT(i, j) EM_2(kEmUENT, i, j)
#define VENT(i, j) EM_2(kEmVENT, i, j)

// ---- saturation specific humidity of level i as the caller gave it, or the reference's bolton_q_sat(T, 100 P, rd, rv) -----------------
RRTMG_EMANUEL_HD double emanuel_qs_in(const EmanuelCall &a, long col, int i) {
#pragma clang fp contract(off)
  const size_t N = (size_t)a.ncol;
  if (a.qs) return a.qs[(size_t)i * N + col];
  const double sc = a.pressure_scale;
  const double T = EM_T(i), p = EM_P(i) * 100.0;
  const double es = 611.2 * exp(17.67 * (T - 273.15) / (T - 29.65));
  const double epsilon = a.rd / a.rv;
  return epsilon * es / (p - (1.0 - epsilon) * es);
}

// ---- _tlift: the parcel from level NK, to the cloud base (KK 1) or from above it to NL (KK 2) -----------------------------------------
RRTMG_EMANUEL_HD void emanuel_tlift(const EmanuelCall &a, long col, int ICB, int NK, int NL, int KK) {
#pragma clang fp contract(off)
  const size_t N = (size_t)a.ncol, CC = (size_t)a.ccol, lc = (size_t)(col - a.col0);
  const double sc = a.pressure_scale;
  const double CPD = a.cpd, CPV = a.cpv, CL = a.cl, RV = a.rv, RD = a.rd, LV0 = a.lv0;
  const double CPVMCL = CL - CPV;
  const double EPS = RD / RV;
  const double EPSI = 1.0 / EPS;
  const double TNK = EM_T(NK), QNK = EM_Q(NK), GZNK = GZ(NK);

  const double AH0 = (CPD * (1.0 - QNK) + CL * QNK) * TNK + QNK * (LV0 - CPVMCL * (TNK - 273.15)) + GZNK;
  const double CPP = CPD * (1.0 - QNK) + QNK * CPV;
  const double CPINV = 1.0 / CPP;

  if (KK == 1) {
    for (int i = 0; i < ICB; ++i) CLW(i) = 0.0;
    for (int i = NK; i < ICB; ++i) {
      const double tpk = TNK - (GZ(i) - GZNK) * CPINV;
      TP(i) = tpk;
      TVP(i) = tpk * (1.0 + QNK * EPSI);
    }
  }

  int NST = ICB, NSB = ICB;
  if (KK == 2) { NST = NL; NSB = ICB + 1; }

  for (int i = NSB; i <= NST; ++i) {
    const double Ti = EM_T(i), Pi = EM_P(i), GZi = GZ(i);
    double TG = Ti;
    double QG = QS(i);
    const double ALV = LV0 - CPVMCL * (Ti - 273.15);
    for (int j = 0; j < 2; ++j) {
      double S = CPD + ALV * ALV * QG / (RV * Ti * Ti);
      S = 1.0 / S;
      const double AHG = CPD * TG + (CL - CPD) * QNK * Ti + ALV * QG + GZi;
      TG = TG + S * (AH0 - AHG);
      TG = emanuel_max(TG, 35.0);
      const double TC = TG - 273.15;
      const double DENOM = 243.5 + TC;
      double ES;
      if (TC >= 0.0) ES = 6.112 * exp(17.67 * TC / DENOM);
      else ES = exp(23.33086 - 6111.72784 / TG + 0.15215 * log(TG));
      QG = EPS * ES / (Pi - ES * (1.0 - EPS));
    }
    const double tpk = (AH0 - (CL - CPD) * QNK * Ti - GZi - ALV * QG) / CPD;
    TP(i) = tpk;
    double clw = QNK - QG;
    clw = emanuel_max(0.0, clw);
    CLW(i) = clw;
    const double RG = QG / (1.0 - QNK);
    TVP(i) = tpk * (1.0 + RG * EPSI);
  }
}

// ---- _convect: one column; the tendencies go to a.ft, a.fq, a.fu, a.fv, the scalars to o ------------------------------------------------
RRTMG_EMANUEL_HD void emanuel_convect(const EmanuelCall &a, long col, EmanuelScalars &o) {
#pragma clang fp contract(off)
  const size_t N = (size_t)a.ncol, CC = (size_t)a.ccol, lc = (size_t)(col - a.col0);
  const int ND = a.nlay, NL = a.nlay - 3, MINORIG = a.minorig;
  const double sc = a.pressure_scale;
  const double CPD = a.cpd, CPV = a.cpv, CL = a.cl, RV = a.rv, RD = a.rd, LV0 = a.lv0, G = a.g, ROWL = a.rowl;
  const double SIGD = a.sigd, SIGS = a.sigs, DELT = a.dt;
  double CBMF = a.cbmf[col];

  for (int i = 0; i < ND; ++i) { EM_FT(i) = 0.0; EM_FQ(i) = 0.0; EM_FU(i) = 0.0; EM_FV(i) = 0.0; }

  const double CPVMCL = CL - CPV;
  const double EPS = RD / RV;
  const double EPSI = 1.0 / EPS;
  const double GINV = 1.0 / G;
  const double DELTI = 1.0 / DELT;

  double PRECIP = 0.0, WD = 0.0, TPRIME = 0.0, QPRIME = 0.0, OUTCAPE = 0.0;
  int IFLAG = 0;
  o.precip = PRECIP; o.wd = WD; o.tprime = TPRIME; o.qprime = QPRIME; o.cape = OUTCAPE; o.iflag = IFLAG; o.cbmf = CBMF;

  const double T0 = EM_T(0), Q0 = EM_Q(0);
  GZ(0) = 0.0;
  CPN(0) = CPD * (1.0 - Q0) + Q0 * CPV;
  H(0) = T0 * CPN(0);
  LV(0) = LV0 - CPVMCL * (T0 - 273.15);
  HM(0) = LV(0) * Q0;
  TV(0) = T0 * (1.0 + Q0 * EPSI - Q0);

  double AHMIN = 1.0e12;
  int IHMIN = NL;
  {
    double Tm = T0, Qm = Q0, Pm = EM_P(0), GZm = 0.0, HMm = HM(0);      // level i - 1
    for (int i = 1; i <= NL; ++i) {
      const double Ti = EM_T(i), Qi = EM_Q(i), Pi = EM_P(i);
      const double TVX = Ti * (1.0 + Qi * EPSI - Qi);
      const double TVY = Tm * (1.0 + Qm * EPSI - Qm);
      const double gz = GZm + 0.5 * RD * (TVX + TVY) * (Pm - Pi) / EM_PH(i);
      GZ(i) = gz;
      const double cpn = CPD * (1.0 - Qi) + CPV * Qi;
      CPN(i) = cpn;
      H(i) = Ti * cpn + gz;
      const double lv = LV0 - CPVMCL * (Ti - 273.15);
      LV(i) = lv;
      const double hm = (CPD * (1.0 - Qi) + CL * Qi) * (Ti - T0) + lv * Qi + gz;
      HM(i) = hm;
      TV(i) = Ti * (1.0 + Qi * EPSI - Qi);
      if ((i + 1) >= MINORIG && hm < AHMIN && hm < HMm) {
        AHMIN = hm;
        IHMIN = i;
      }
      Tm = Ti; Qm = Qi; Pm = Pi; GZm = gz; HMm = hm;
    }
  }

  IHMIN = IHMIN < NL - 1 ? IHMIN : NL - 1;
  double AHMAX = 0.0;
  int NK = 0;
  for (int i = MINORIG - 1; i <= IHMIN; ++i) {
    const double hm = HM(i);
    if (hm > AHMAX) { NK = i; AHMAX = hm; }
  }

  const double TNK = EM_T(NK), QNK = EM_Q(NK), UNK = EM_U(NK), VNK = EM_V(NK), PNK = EM_P(NK);
  if (TNK < 250.0 || QNK <= 0.0 || IHMIN == (NL - 1)) {
    o.iflag = 0; o.cbmf = 0.0;
    return;
  }

  const double RH = QNK / emanuel_qs_in(a, col, NK);
  const double CHI = TNK / (1669.0 - 122.0 * RH - TNK);
  const double PLCL = PNK * pow(RH, CHI);

  if (PLCL < 200.0 || PLCL >= 2000.0) {
    o.iflag = 2; o.cbmf = 0.0;
    return;
  }

  int ICB = NL - 1;
  for (int i = NK + 1; i <= NL; ++i)
    if (EM_P(i) < PLCL) ICB = ICB < i ? ICB : i;

  if (ICB >= (NL - 1)) {
    o.iflag = 3; o.cbmf = 0.0;
    return;
  }

  for (int i = 0; i <= NL; ++i) QS(i) = emanuel_qs_in(a, col, i);
  for (int i = 0; i < NK; ++i) { TVP(i) = 0.0; TP(i) = 0.0; }      // (np.zeros; never read, kept defined)
  emanuel_tlift(a, col, ICB, NK, NL, 1);
  for (int i = NK; i <= ICB; ++i) TVP(i) -= TP(i) * QNK;

  if (CBMF == 0.0 && TVP(ICB) <= (TV(ICB) - a.dtmax)) {
    o.iflag = 0;
    return;
  }

  IFLAG = 1;

  emanuel_tlift(a, col, ICB, NK, NL, 2);

  for (int i = 0; i <= NK; ++i) EP(i) = 0.0;
  for (int i = NK + 1; i <= NL; ++i) {
    const double TCA = TP(i) - 273.15;
    double ELACRIT = TCA >= 0.0 ? a.elcrit : a.elcrit * (1.0 - TCA / a.tlcrit);
    ELACRIT = emanuel_max(ELACRIT, 0.0);
    const double EPMAX = 0.999;
    double ep = EPMAX * (1.0 - ELACRIT / emanuel_max(CLW(i), 1.0e-8));
    ep = emanuel_max(emanuel_min(ep, EPMAX), 0.0);
    EP(i) = ep;
  }

  for (int i = ICB + 1; i <= NL; ++i) TVP(i) -= TP(i) * QNK;

  for (int i = 0; i <= NL + 1; ++i) {
    HP(i) = i <= NL ? H(i) : 0.0;
    NENT(i) = 0.0; WATER(i) = 0.0; EVAP(i) = 0.0; WT(i) = a.omtsnow; MP(i) = 0.0; M(i) = 0.0;
    LVCP(i) = i <= NL ? LV(i) / CPN(i) : 0.0;
    QP(i) = 0.0; UP(i) = 0.0; VP(i) = 0.0;
  }
  // index NL + 1 of the reference's zero-filled arrays: GZ[INB+1] is read (times AMP1 = 0) where INB == NL
  GZ(NL + 1) = 0.0; CPN(NL + 1) = 0.0; H(NL + 1) = 0.0; LV(NL + 1) = 0.0; HM(NL + 1) = 0.0; TV(NL + 1) = 0.0;
  TVP(NL + 1) = 0.0; TP(NL + 1) = 0.0; CLW(NL + 1) = 0.0; EP(NL + 1) = 0.0;
  QP(0) = Q0; UP(0) = EM_U(0); VP(0) = EM_V(0);
  for (int i = 1; i <= NL; ++i) { QP(i) = EM_Q(i - 1); UP(i) = EM_U(i - 1); VP(i) = EM_V(i - 1); }

  double CAPE = 0.0, CAPEM = 0.0;
  int INB = ICB + 1;
  int INB1 = INB;
  double BYP = 0.0;
  for (int i = ICB + 1; i < NL; ++i) {
    const double BY = (TVP(i) - TV(i)) * (EM_PH(i) - EM_PH(i + 1)) / EM_P(i);
    CAPE += BY;
    if (BY >= 0.0) INB1 = i + 1;
    if (CAPE > 0.0) {
      INB = i + 1;
      BYP = (TVP(i + 1) - TV(i + 1)) * (EM_PH(i + 1) - EM_PH(i + 2)) / EM_P(i + 1);
      CAPEM = CAPE;
    }
  }
  INB = INB > INB1 ? INB : INB1;
  CAPE = CAPEM + BYP;
  const double DEFRAC = emanuel_max(CAPEM - CAPE, 0.001);
  const double FRAC = emanuel_min(emanuel_max(-CAPE / DEFRAC, 0.0), 1.0);
  OUTCAPE = CAPE;

  const double HNK = H(NK);
  for (int i = ICB; i <= INB; ++i) HP(i) = HNK + (LV(i) + (CPD - CPV) * EM_T(i)) * EP(i) * CLW(i);

  const double TVPPLCL = TVP(ICB - 1) - RD * TVP(ICB - 1) * (EM_P(ICB - 1) - PLCL) / (CPN(ICB - 1) * EM_P(ICB - 1));
  const double TVAPLCL = TV(ICB) + (TVP(ICB) - TVP(ICB + 1)) * (PLCL - EM_P(ICB)) / (EM_P(ICB) - EM_P(ICB + 1));
  double DTPBL = 0.0;
  for (int i = NK; i < ICB; ++i) DTPBL += (TVP(i) - TV(i)) * (EM_PH(i) - EM_PH(i + 1));
  DTPBL /= EM_PH(NK) - EM_PH(ICB);
  const double DTMA = TVPPLCL - TVAPLCL + a.dtmax + DTPBL;

  const double CBMFOLD = CBMF;
  const double DAMPS = a.damp * DELT / a.delt0;
  CBMF = (1.0 - DAMPS) * CBMF + 0.1 * a.alpha * DTMA;
  CBMF = emanuel_max(CBMF, 0.0);

  o.iflag = IFLAG; o.cbmf = CBMF; o.cape = OUTCAPE;
  if (CBMF == 0.0 && CBMFOLD == 0.0) return;

  // the 2-D block of this column: rows ICB+1 .. INB, columns ICB .. INB (SIJ is written in full by the first loop below)
  for (int i = ICB + 1; i <= INB; ++i)
    for (int j = ICB; j <= INB; ++j) {
      MENT(i, j) = 0.0; ELIJ(i, j) = 0.0;
      QENT(i, j) = EM_Q(j); UENT(i, j) = EM_U(j); VENT(i, j) = EM_V(j);
    }

  M(ICB) = 0.0;
  double DBOSUM = 0.0;
  for (int i = ICB + 1; i <= INB; ++i) {
    const int k = i < INB1 ? i : INB1;
    const double DBO = fabs(TV(k) - TVP(k)) + a.entp * 0.02 * (EM_PH(k) - EM_PH(k + 1));
    DBOSUM += DBO;
    M(i) = CBMF * DBO;
  }
  if (DBOSUM > 0)
    for (int i = ICB + 1; i <= INB; ++i) M(i) /= DBOSUM;

  for (int i = ICB + 1; i <= INB; ++i) {
    const double Qi = EM_Q(i), Ui = EM_U(i), Vi = EM_V(i), Hi = H(i), HPi = HP(i), Mi = M(i);
    const double QTI = QNK - EP(i) * CLW(i);
    double nent = NENT(i);
    for (int j = ICB; j <= INB; ++j) {
      const double Tj = EM_T(j), Qj = EM_Q(j), QSj = QS(j), LVj = LV(j);
      const double BF2 = 1.0 + LVj * LVj * QSj / (RV * Tj * Tj * CPD);
      double ANUM = H(j) - HPi + (CPV - CPD) * Tj * (QTI - Qj);
      double DENOM = Hi - HPi + (CPD - CPV) * (Qi - QTI) * Tj;
      double DEI = DENOM;
      if (fabs(DEI) < 0.01) DEI = 0.01;
      double s = ANUM / DEI;
      if (j == i) s = 1.0;      // the reference sets SIJ[i][i] = 1 behind every SIJ[i][j] = ANUM / DEI, this one included
      double ALTEM = (s * Qi + (1.0 - s) * QTI - QSj) / BF2;
      const double CWAT = CLW(j) * (1.0 - EP(j));
      if ((s < 0.0 || s > 1.0 || ALTEM > CWAT) && j > i) {
        ANUM -= LVj * (QTI - QSj - CWAT * BF2);
        DENOM += LVj * (Qi - QTI);
        if (fabs(DENOM) < 0.01) DENOM = 0.01;
        s = ANUM / DENOM;
        ALTEM = s * Qi + (1.0 - s) * QTI - QSj - (BF2 - 1.0) * CWAT;
      }
      if (0.0 < s && s < 0.9) {
        QENT(i, j) = s * Qi + (1.0 - s) * QTI;
        UENT(i, j) = s * Ui + (1.0 - s) * UNK;
        VENT(i, j) = s * Vi + (1.0 - s) * VNK;
        ELIJ(i, j) = emanuel_max(0.0, ALTEM);
        MENT(i, j) = Mi / (1.0 - s);
        nent += 1.0;
      }
      SIJ(i, j) = emanuel_min(emanuel_max(s, 0.0), 1.0);
    }
    SIJ(i, i) = 1.0;      // (the reference sets it at every j and, for i == INB, once more behind the loop)
    NENT(i) = nent;
    if (nent == 0.0) {
      MENT(i, i) = Mi;
      QENT(i, i) = QNK - EP(i) * CLW(i);
      UENT(i, i) = UNK;
      VENT(i, i) = VNK;
      ELIJ(i, i) = CLW(i);
      SIJ(i, i) = 1.0;
    }
  }

  for (int i = ICB + 1; i <= INB; ++i) {
    if (NENT(i) != 0.0) {
      const double Qi = EM_Q(i), QSi = QS(i), LVi = LV(i);
      const double QP1 = QNK - EP(i) * CLW(i);
      const double ANUM = H(i) - HP(i) - LVi * (QP1 - QSi);
      double DENOM = H(i) - HP(i) + LVi * (Qi - QP1);
      if (fabs(DENOM) < 0.01) DENOM = 0.01;
      double SCRIT = ANUM / DENOM;
      const double ALT = QP1 - QSi + SCRIT * (Qi - QP1);
      if (ALT < 0.0) SCRIT = 1.0;
      SCRIT = emanuel_max(SCRIT, 0.0);
      double ASIJ = 0.0;
      double SMIN = 1.0;
      for (int j = ICB; j <= INB; ++j) {
        const double sij = SIJ(i, j);
        if (0.0 < sij && sij < 0.9) {
          const double s_up = j + 1 <= INB ? SIJ(i, j + 1) : 0.0;      // SIJ[i][INB+1] and SIJ[i][ICB-1] are never written: 0
          const double s_dn = j - 1 >= ICB ? SIJ(i, j - 1) : 0.0;
          double SMID, SJMAX, SJMIN;
          if (j > i) {
            SMID = emanuel_min(sij, SCRIT);
            SJMAX = SMID;
            SJMIN = SMID;
            if (SMID < SMIN && s_up < SMID) {
              SMIN = SMID;
              SJMAX = emanuel_min(emanuel_min(s_up, sij), SCRIT);
              SJMIN = emanuel_min(emanuel_max(s_dn, sij), SCRIT);
            }
          } else {
            SJMAX = emanuel_max(s_up, SCRIT);
            SMID = emanuel_max(sij, SCRIT);
            SJMIN = emanuel_max(s_dn, SCRIT);      // (j > 0 always: j >= ICB >= 1)
          }
          const double dph = EM_PH(j) - EM_PH(j + 1);
          ASIJ += (fabs(SJMAX - SMID) + fabs(SJMIN - SMID)) * dph;
          MENT(i, j) *= (fabs(SJMAX - SMID) + fabs(SJMIN - SMID)) * dph;
        }
      }
      ASIJ = emanuel_max(1.0e-21, ASIJ);
      double total = 0.0;
      for (int j = ICB; j <= INB; ++j) {
        const double m = MENT(i, j) / ASIJ;
        MENT(i, j) = m;
        total = j == ICB ? m : total + m;
      }
      if (total < 1.0e-18) {
        NENT(i) = 0.0;
        MENT(i, i) = M(i);
        QENT(i, i) = QNK - EP(i) * CLW(i);
        UENT(i, i) = UNK;
        VENT(i, i) = VNK;
        ELIJ(i, i) = CLW(i);
        SIJ(i, i) = 1.0;
      }
    }
  }

  if (EP(INB) >= 0.0001) {
    int JTT = 0;
    const double P0 = EM_P(0);
    for (int i = INB; i >= 0; --i) {
      const double Ti = EM_T(i), Qi = EM_Q(i), Pi = EM_P(i), PHi = EM_PH(i), PHi1 = EM_PH(i + 1), QSi = QS(i), EPi = EP(i), CLWi = CLW(i);
      double WDTRAIN = G * EPi * M(i) * CLWi;
      if (i >= ICB)
        for (int j = ICB + 1; j < i; ++j) WDTRAIN += G * emanuel_max(0.0, ELIJ(j, i) - (1.0 - EPi) * CLWi) * MENT(j, i);
      const double COEFF = Ti > 273.0 ? a.coeffr : a.coeffs;
      const double wt = Ti > 273.0 ? a.omtrain : a.omtsnow;
      WT(i) = wt;
      const double AFAC = emanuel_max(COEFF * PHi * (QSi - 0.5 * (Qi + QP(i + 1))) / (1.0e4 + 2.0e3 * PHi * QSi), 0.0);
      const double SIGT = emanuel_min(emanuel_max(SIGS, 0.0), 1.0);
      const double B6 = 100.0 * (PHi - PHi1) * SIGT * AFAC / wt;
      const double C6 = (WATER(i + 1) * WT(i + 1) + WDTRAIN / SIGD) / wt;
      const double REVAP = 0.5 * (-B6 + sqrt(B6 * B6 + 4.0 * C6));
      EVAP(i) = SIGT * AFAC * REVAP;
      WATER(i) = REVAP * REVAP;
      if (i > 0) {
        const double DHDP = emanuel_max((H(i) - H(i - 1)) / (EM_P(i - 1) - Pi), 10.0);
        double mp = 100.0 * GINV * LV(i) * SIGD * EVAP(i) / DHDP;
        const double FAC = 20.0 / (EM_PH(i - 1) - PHi);
        mp = (FAC * MP(i + 1) + mp) / (1.0 + FAC);
        MP(i) = mp;
        if (Pi > (0.949 * P0)) {
          JTT = JTT > i ? JTT : i;
          MP(i) = MP(JTT) * (P0 - Pi) / (P0 - EM_P(JTT));
        }
      }
      if (i != INB) {
        const double QSTM = i == 0 ? QS(0) : QS(i - 1);
        const double MPi = MP(i), MPi1 = MP(i + 1);
        if (MPi > MPi1) {
          const double RAT = MPi1 / MPi;
          QP(i) = QP(i + 1) * RAT + Qi * (1.0 - RAT) + 100.0 * GINV * SIGD * (PHi - PHi1) * (EVAP(i) / MPi);
          UP(i) = UP(i + 1) * RAT + EM_U(i) * (1.0 - RAT);
          VP(i) = VP(i + 1) * RAT + EM_V(i) * (1.0 - RAT);
        } else if (MPi1 > 0.0) {
          QP(i) = (GZ(i + 1) - GZ(i) + QP(i + 1) * (LV(i + 1) + EM_T(i + 1) * (CL - CPD)) + CPD * (EM_T(i + 1) - Ti)) / (LV(i) + Ti * (CL - CPD));
          UP(i) = UP(i + 1);
          VP(i) = VP(i + 1);
        }
        QP(i) = emanuel_max(emanuel_min(QP(i), QSTM), 0.0);
      }
    }
    PRECIP += WT(0) * SIGD * WATER(0) * 3600.0 * 24000.0 / (ROWL * G);
  }

  WD = a.beta * fabs(MP(ICB)) * 0.01 * RD * EM_T(ICB) / (SIGD * EM_P(ICB));
  QPRIME = 0.5 * (QP(0) - Q0);
  TPRIME = LV0 * QPRIME / CPD;
  {
    const double DPINV = 0.01 / (EM_PH(0) - EM_PH(1));
    double AM = 0.0;
    if (NK == 0)
      for (int i = 1; i <= INB; ++i) AM = i == 1 ? M(i) : AM + M(i);
    if ((2.0 * G * DPINV * AM) >= DELTI) IFLAG = 4;
    const double T1 = EM_T(1), Q1 = EM_Q(1), U0 = EM_U(0), U1 = EM_U(1), V0 = EM_V(0), V1 = EM_V(1);
    EM_FT(0) += G * DPINV * AM * (T1 - T0 + (GZ(1) - GZ(0)) / CPN(0)) - LVCP(0) * SIGD * EVAP(0)
                + SIGD * WT(1) * (CL - CPD) * WATER(1) * (T1 - T0) * DPINV / CPN(0);
    EM_FQ(0) += G * MP(1) * (QP(1) - Q0) * DPINV + SIGD * EVAP(0) + G * AM * (Q1 - Q0) * DPINV;
    EM_FU(0) += G * DPINV * (MP(1) * (UP(1) - U0) + AM * (U1 - U0));
    EM_FV(0) += G * DPINV * (MP(1) * (VP(1) - V0) + AM * (V1 - V0));
    // (MENT[j][0], j = 1 .. INB: column 0 lies below every cloud base -- the reference adds 0 * (Q[0] - Q[0]))
  }

  for (int i = 1; i <= INB; ++i) {
    const double Ti = EM_T(i), Qi = EM_Q(i), Ui = EM_U(i), Vi = EM_V(i);
    const double Tm = EM_T(i - 1), Qm = EM_Q(i - 1), Um = EM_U(i - 1), Vm = EM_V(i - 1);
    const double Tp = EM_T(i + 1), Qp = EM_Q(i + 1), Upl = EM_U(i + 1), Vpl = EM_V(i + 1);
    const double DPINV = 0.01 / (EM_PH(i) - EM_PH(i + 1));
    const double CPINV = 1.0 / CPN(i);
    double AMP1 = 0.0;
    if (i >= NK)
      for (int k = i + 1; k <= INB + 1; ++k) AMP1 = k == i + 1 ? M(k) : AMP1 + M(k);
    for (int k = ICB + 1; k <= i; ++k) {      // rows below ICB + 1 hold nothing; column INB + 1 neither
      double row = 0.0;
      for (int j = i + 1; j <= INB; ++j) row = j == i + 1 ? MENT(k, j) : row + MENT(k, j);
      AMP1 += row;
    }
    if ((2.0 * G * DPINV * AMP1) >= DELTI) IFLAG = 4;
    double AD = 0.0;
    for (int k = ICB; k < i; ++k) {           // columns below ICB hold nothing
      double colsum = 0.0;
      const int r0 = i > ICB + 1 ? i : ICB + 1;
      for (int r = r0; r <= INB; ++r) colsum = r == r0 ? MENT(r, k) : colsum + MENT(r, k);
      AD += colsum;
    }
    double ft = EM_FT(i), fq = EM_FQ(i), fu = EM_FU(i), fv = EM_FV(i);
    ft += G * DPINV * (AMP1 * (Tp - Ti + (GZ(i + 1) - GZ(i)) * CPINV) - AD * (Ti - Tm + (GZ(i) - GZ(i - 1)) * CPINV)) - SIGD * LVCP(i) * EVAP(i);
    if (i >= ICB + 1) ft += G * DPINV * MENT(i, i) * (HP(i) - H(i) + Ti * (CPV - CPD) * (Qi - QENT(i, i))) * CPINV;
    ft += SIGD * WT(i + 1) * (CL - CPD) * WATER(i + 1) * (Tp - Ti) * DPINV * CPINV;
    fq += G * DPINV * (AMP1 * (Qp - Qi) - AD * (Qi - Qm));
    fu += G * DPINV * (AMP1 * (Upl - Ui) - AD * (Ui - Um));
    fv += G * DPINV * (AMP1 * (Vpl - Vi) - AD * (Vi - Vm));
    if (i >= ICB) {
      const double EPi = EP(i), CLWi = CLW(i);
      for (int k = ICB + 1; k < i; ++k) {
        const double ment = MENT(k, i);
        const double AWAT = emanuel_max(ELIJ(k, i) - (1.0 - EPi) * CLWi, 0.0);
        fq += G * DPINV * ment * (QENT(k, i) - AWAT - Qi);
        fu += G * DPINV * ment * (UENT(k, i) - Ui);
        fv += G * DPINV * ment * (VENT(k, i) - Vi);
      }
      for (int k = i > ICB + 1 ? i : ICB + 1; k <= INB; ++k) {
        const double ment = MENT(k, i);
        fq += G * DPINV * ment * (QENT(k, i) - Qi);
        fu += G * DPINV * ment * (UENT(k, i) - Ui);
        fv += G * DPINV * ment * (VENT(k, i) - Vi);
      }
    }
    fq += SIGD * EVAP(i) + G * (MP(i + 1) * (QP(i + 1) - Qi) - MP(i) * (QP(i) - Qm)) * DPINV;
    fu += G * (MP(i + 1) * (UP(i + 1) - Ui) - MP(i) * (UP(i) - Um)) * DPINV;
    fv += G * (MP(i + 1) * (VP(i + 1) - Vi) - MP(i) * (VP(i) - Vm)) * DPINV;
    EM_FT(i) = ft; EM_FQ(i) = fq; EM_FU(i) = fu; EM_FV(i) = fv;
  }

  {
    const double ratio = (EM_PH(INB) - EM_PH(INB + 1)) / (EM_PH(INB - 1) - EM_PH(INB));
    const double FQOLD = EM_FQ(INB);
    EM_FQ(INB) *= 1.0 - FRAC;
    EM_FQ(INB - 1) += FRAC * FQOLD * ratio * LV(INB) / LV(INB - 1);
    const double FTOLD = EM_FT(INB);
    EM_FT(INB) *= 1.0 - FRAC;
    EM_FT(INB - 1) += FRAC * FTOLD * ratio * CPN(INB) / CPN(INB - 1);
    const double FUOLD = EM_FU(INB);
    EM_FU(INB) *= 1.0 - FRAC;
    EM_FU(INB - 1) += FRAC * FUOLD * ratio;
    const double FVOLD = EM_FV(INB);
    EM_FV(INB) *= 1.0 - FRAC;
    EM_FV(INB - 1) += FRAC * FVOLD * ratio;
  }

  double ENTS = 0.0, UAV = 0.0, VAV = 0.0;
  for (int i = 0; i <= INB; ++i) {
    const double dph = EM_PH(i) - EM_PH(i + 1);
    const double e = (CPN(i) * EM_FT(i) + LV(i) * EM_FQ(i)) * dph, x = EM_FU(i) * dph, y = EM_FV(i) * dph;
    ENTS = i == 0 ? e : ENTS + e;
    UAV = i == 0 ? x : UAV + x;
    VAV = i == 0 ? y : VAV + y;
  }
  const double depth = EM_PH(0) - EM_PH(INB + 1);
  ENTS = ENTS / depth; UAV = UAV / depth; VAV = VAV / depth;
  for (int i = 0; i <= INB; ++i) {
    EM_FT(i) -= ENTS / CPN(i);
    EM_FU(i) = (1.0 - a.cu) * (EM_FU(i) - UAV);
    EM_FV(i) = (1.0 - a.cu) * (EM_FV(i) - VAV);
  }

  o.precip = PRECIP; o.wd = WD; o.tprime = TPRIME; o.qprime = QPRIME; o.cbmf = CBMF; o.cape = OUTCAPE; o.iflag = IFLAG;
}

// ---- one column of a launch: the rule, then the scalars and the K/day copy of the heating ---------------------------------------------
RRTMG_EMANUEL_HD void emanuel_column(const EmanuelCall &a, long col) {
#pragma clang fp contract(off)
  EmanuelScalars o;
  emanuel_convect(a, col, o);
  if (a.precip) a.precip[col] = o.precip;
  if (a.wd) a.wd[col] = o.wd;
  if (a.tprime) a.tprime[col] = o.tprime;
  if (a.qprime) a.qprime[col] = o.qprime;
  if (a.cape) a.cape[col] = o.cape;
  if (a.iflag) a.iflag[col] = o.iflag;
  a.cbmf_out[col] = o.cbmf;
  if (a.ft_per_day) {
    const size_t N = (size_t)a.ncol;
    for (int i = 0; i < a.nlay; ++i) a.ft_per_day[(size_t)i * N + col] = a.ft[(size_t)i * N + col] * 86400.0;
  }
}

#undef EM_T
#undef EM_Q
#undef EM_U
#undef EM_V
#undef EM_P
#undef EM_PH
#undef EM_FT
#undef EM_FQ
#undef EM_FU
#undef EM_FV
#undef EM_1
#undef EM_2
#undef GZ
#undef CPN
#undef H
#undef LV
#undef HM
#undef TV
#undef TVP
#undef TP
#undef CLW
#undef EP
#undef HP
#undef WATER
#undef EVAP
#undef WT
#undef MP
#undef M
#undef LVCP
#undef QP
#undef UP
#undef VP
#undef QS
#undef NENT
#undef MENT
#undef QENT
#undef ELIJ
#undef SIJ
#undef UENT
#undef VENT

}  // namespace rrtmg
