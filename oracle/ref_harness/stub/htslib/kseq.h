// oracle/ref_harness/stub/htslib/kseq.h -- TEST INFRASTRUCTURE ONLY.
// Empty on purpose: the reference's MinCount.h includes "htslib/kseq.h" and uses nothing from it, so this stand-in on the include path lets
// ref_harness/minimizers_ref.cpp compile StoreMinimizers where it lies without htslib.
