/* TEST INFRASTRUCTURE: stand-in for htslib's sam.h with only the names the reference's math headers mention, so that `make -C oracle ref_math` compiles them without htslib. */
#ifndef UVC_REF_SHIM_SAM_H
#define UVC_REF_SHIM_SAM_H
#include <stdint.h>
typedef struct { int32_t tid; int64_t pos; } bam1_core_t;
typedef struct { bam1_core_t core; char *qname_; } bam1_t;
#define bam_get_qname(b) ((b)->qname_)
/* CIGAR operation codes of the SAM specification, "MIDNSHP=XB" */
enum { BAM_CMATCH = 0, BAM_CINS = 1, BAM_CDEL = 2, BAM_CREF_SKIP = 3, BAM_CSOFT_CLIP = 4, BAM_CHARD_CLIP = 5, BAM_CPAD = 6, BAM_CEQUAL = 7, BAM_CDIFF = 8, BAM_CBACK = 9 };
#endif
