/* TEST INFRASTRUCTURE: stand-in for htslib's vcf.h (see sam.h beside it): the record type is only ever held by pointer. */
typedef struct bcf1_t bcf1_t;
